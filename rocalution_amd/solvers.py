"""Krylov solvers / preconditioners: Python handles onto the compiled C++ layer
(include/rocalution/solvers.hpp, instantiated in csrc/capi_solvers.cpp).

Class and method names follow the reference (src/solvers/solver.hpp:179-444): SetOperator,
SetPreconditioner, Init, Build, Solve, Clear, GetIterationCount, GetCurrentResidual,
GetSolverStatus, GMRES.SetBasisSize, MixedPrecisionDC.Set.  The numerical work happens in the
library; nothing here computes.
"""
import ctypes as C

import numpy as np

from . import capi
from .capi import (PC_AS, PC_RAS, PC_BLOCK, PC_GS, PC_IC, PC_ILU0, PC_SAAMG, PC_UAAMG, PC_JACOBI, PC_MCGS, PC_MCILU, PC_MCSGS, PC_MULTIELIM, PC_NONE, PC_RSAMG, PC_SGS, PC_TNS, SOLVER_BICGSTAB,
                   SOLVER_BICGSTABL,
                   SOLVER_CG, SOLVER_CHEBYSHEV, SOLVER_CR, SOLVER_FCG, SOLVER_FGMRES, SOLVER_FIXEDPOINT, SOLVER_GMRES,
                   SOLVER_IDR, SOLVER_QMRCGSTAB)


def _lib():
    return capi.load()


TriSolverAlg_Default, TriSolverAlg_Iterative = 0, 1


class SolverDescr:
    """triangular-solve strategy of a preconditioner (solver.hpp:82-148): defaults direct, 30 sweeps, 1e-3, tol on"""

    def __init__(self):
        self.alg, self.max_iter, self.tol, self.use_tol = TriSolverAlg_Default, 30, 1e-3, True

    def SetTriSolverAlg(self, alg):
        self.alg = int(alg)

    def SetIterativeSolverMaxIteration(self, n):
        self.max_iter = int(n)

    def SetIterativeSolverTolerance(self, tol):
        self.tol = float(tol)

    def EnableIterativeSolverTolerance(self):
        self.use_tol = True

    def DisableIterativeSolverTolerance(self):
        self.use_tol = False


class _Precond:
    kind = PC_NONE

    def __init__(self):
        self.precond_format = None
        self.descr = None

    def SetSolverDescriptor(self, descr):
        self.descr = descr

    def SetPrecondMatrixFormat(self, fmt):
        self.precond_format = int(fmt)


class Jacobi(_Precond):
    kind = PC_JACOBI


class ILU(_Precond):
    kind = PC_ILU0

    def Set(self, p, level=True):
        """ILU(p) (preconditioner.cpp:420-447): fill levels on the pattern of A^(p+1), or (level=False) that whole pattern"""
        if p < 0:
            raise ValueError("ILU(p): p >= 0")
        self.params = (float(p), 1.0 if level else 0.0, 0.0)


class GS(_Precond):
    """Gauss-Seidel: LSolve on the matrix (preconditioner.cpp:206-257)"""
    kind = PC_GS


class SGS(_Precond):
    """symmetric Gauss-Seidel: LSolve, diagonal scaling, USolve (preconditioner.cpp:302-379)"""
    kind = PC_SGS


class IC(_Precond):
    """incomplete Cholesky, zero fill-in (preconditioner.cpp:826-925): ICFactorize on ExtractL, LLSolve"""
    kind = PC_IC


class UAAMG(_Precond):
    """unsmoothed-aggregation AMG as a preconditioner (unsmoothed_amg.cpp), PMIS coarsening on the device, default
    FixedPoint(2/3)+Jacobi smoothers and CG coarse solver, coarsest level <= 300 rows"""
    kind = PC_UAAMG


class SAAMG(_Precond):
    """smoothed-aggregation AMG as a preconditioner (smoothed_amg.cpp), PMIS coarsening on the device"""
    kind = PC_SAAMG


Greedy, PMIS = 0, 1
Direct, ExtPI = 0, 1


class RugeStuebenAMG(_Precond):
    """classical (Ruge-Stueben) AMG as a preconditioner (ruge_stueben_amg.cpp): defaults as the reference's class --
    threshold 0.25, Greedy coarsening (a sequential sweep on the host; PMIS runs on the device), Direct interpolation,
    FF1 limit off, coarsest level <= 300 rows"""
    kind = PC_RSAMG

    def __init__(self):
        super().__init__()
        self._eps, self._strat, self._interp, self._ff1, self._coarsest = 0.25, Greedy, Direct, False, 0
        self._pack()

    def _pack(self):
        self.params = (float(self._eps), float(self._strat + 2 * self._interp + 4 * int(self._ff1)), float(self._coarsest))

    def SetStrengthThreshold(self, eps):
        self._eps = float(eps); self._pack()

    def SetCoarseningStrategy(self, strat):
        if strat not in (Greedy, PMIS):
            raise ValueError("RugeStuebenAMG: Greedy (0) or PMIS (1)")
        self._strat = int(strat); self._pack()

    def SetInterpolationType(self, interp):
        if interp not in (Direct, ExtPI):
            raise ValueError("RugeStuebenAMG: Direct (0) or ExtPI (1)")
        self._interp = int(interp); self._pack()

    def SetInterpolationFF1Limit(self, ff1):
        self._ff1 = bool(ff1); self._pack()

    def SetCoarsestLevel(self, rows):
        self._coarsest = int(rows); self._pack()


class TNS(_Precond):
    """truncated Neumann series (preconditioner_ai.cpp:476-713): M^-1 = (I - K^T + K^T^2) D^-1 (I - K + K^2) with
    K = strict_lower(A) D^-1.  impl=True: the products at every Solve (form: -1 the library's choice, 0 stored K and K^T,
    1 matrix-free on a bitwise symmetric operator); impl=False: M^-1 assembled as one matrix.  SetPrecondMatrixFormat
    converts the stored matrices and selects the stored form"""
    kind = PC_TNS

    def __init__(self, impl=True, form=-1):
        super().__init__()
        if int(form) not in (-1, 0, 1):
            raise ValueError("TNS: form is -1 (auto), 0 (stored) or 1 (matrix-free)")
        self.params = (1.0 if impl else 0.0, float(int(form)), 0.0)

    def Set(self, impl):
        self.params = (1.0 if impl else 0.0, self.params[1], 0.0)


class TNSPlan:
    """the TNS apply on its own (ramd_tns_*): Build on a LocalMatrix, Apply(rhs, x); the kernel tests drive this"""
    STORED, MATRIX_FREE, EXPLICIT = 0, 1, 2

    def __init__(self, mat, impl=True, form=-1):
        self._h = C.c_void_p()
        self._mat = mat  # the matrix-free form reads the operator: keep it alive
        capi.check(_lib().ramd_tns_build(mat._h, 1 if impl else 0, int(form), C.byref(self._h)))

    def __del__(self):
        try:
            self.Clear()
        except Exception:
            pass

    def Clear(self):
        if self._h:
            _lib().ramd_tns_destroy(self._h)
            self._h = None

    def ConvertTo(self, fmt):
        capi.check(_lib().ramd_tns_convert(self._h, int(fmt)))

    def Apply(self, rhs, x):
        capi.check(_lib().ramd_tns_apply(self._h, rhs._h, x._h))

    def Info(self):
        """-> dict(form, impl, symmetric, rows, nnz, format, format_t)"""
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_tns_info(self._h, out))
        keys = ("form", "impl", "symmetric", "rows", "nnz", "format", "format_t")
        return dict(zip(keys, [int(v) for v in out[:7]]))


class MultiElimination(_Precond):
    """multi-elimination ILU (preconditioner_multielimination.cpp): an independent set of rows is eliminated without a
    triangular solve and the Schur complement goes to `last` (any local preconditioner but the AMG ones; default Jacobi)
    or, for level > 1, to another elimination.  `last` is taken by its kind, with that kind's defaults: an object that
    carries settings of its own is refused.  drop_off > 0 compresses the Schur complements.  SetPrecondMatrixFormat
    converts E and F and selects the stepwise apply"""
    kind = PC_MULTIELIM

    def __init__(self, last=None, level=1, drop_off=0.0):
        super().__init__()
        self.Set(last if last is not None else Jacobi(), level, drop_off)

    def Set(self, last, level, drop_off=0.0):
        if int(level) < 0 or float(drop_off) < 0:
            raise ValueError("MultiElimination: level >= 0 and drop_off >= 0")
        if vars(last) != vars(type(last)()):
            raise ValueError("MultiElimination: the last-block solver is taken by kind, with its defaults; settings of the "
                             "%s object (parameters, format, descriptor) would not reach it" % type(last).__name__)
        self.last = last
        self.params = (float(int(level)), float(drop_off), float(last.kind))


class MEPlan:
    """one elimination level on its own (ramd_me_*): Build on a LocalMatrix, Schur() hands the Schur complement out,
    Down(rhs, rhs2) and Up(rhs, x2, x) are the two halves of the apply; the kernel tests drive this"""
    STEPWISE, FUSED = 0, 1

    def __init__(self, mat, drop_off=0.0, form=-1, max_rounds=0):
        self._h = C.c_void_p()
        self.dtype = mat.dtype
        capi.check(_lib().ramd_me_build(mat._h, float(drop_off), int(form), int(max_rounds), C.byref(self._h)))

    def __del__(self):
        try:
            self.Clear()
        except Exception:
            pass

    def Clear(self):
        if self._h:
            _lib().ramd_me_destroy(self._h)
            self._h = None

    def Schur(self):
        """-> LocalMatrix AA = C - E D^-1 F (once: the plan gives it away)"""
        from . import LocalMatrix
        h = capi.mat_t()
        capi.check(_lib().ramd_me_schur(self._h, C.byref(h)))
        out = LocalMatrix(self.dtype)
        _lib().ramd_mat_destroy(out._h)
        out._h = h
        return out

    def ConvertTo(self, fmt):
        capi.check(_lib().ramd_me_convert(self._h, int(fmt)))

    def Down(self, rhs, rhs2):
        capi.check(_lib().ramd_me_down(self._h, rhs._h, rhs2._h))

    def Up(self, rhs, x2, x):
        capi.check(_lib().ramd_me_up(self._h, rhs._h, x2._h, x._h))

    def Info(self):
        """-> dict(form, rows, size, host_sweep, rounds, symmetric, nnz_ef, nnz_aa)"""
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_me_info(self._h, out))
        keys = ("form", "rows", "size", "host_sweep", "rounds", "symmetric", "nnz_ef", "nnz_aa")
        return dict(zip(keys, [int(v) for v in out]))


def as_layout(n, nb, overlap):
    """-> (pos, sizes): the blocks of AS / RAS on n rows (ramd_as_layout: host code, no device); raises where the layout is
    refused"""
    k = max(int(nb), 1)
    pos, sizes = (C.c_int * k)(), (C.c_int * k)()
    capi.check(_lib().ramd_as_layout(int(n), int(nb), int(overlap), pos, sizes))
    return np.array(pos[:k], dtype=np.int64), np.array(sizes[:k], dtype=np.int64)


class AS(_Precond):
    """additive Schwarz (preconditioner_as.cpp): nb overlapping diagonal blocks, a solver `local` on each, the results added
    with the reference's weights.  `local` is taken by its kind (those MultiElimination takes as its last block; default
    Jacobi), one object per block with that kind's defaults: an object that carries settings of its own is refused -- but
    for ILU.Set(p, level), which reaches every block.  SetForm: -1 the library's choice, 0 stepwise (the reference's
    calls), 1 fused (restriction and prolongation in one launch each), 2 stacked (one local solve on the direct sum of the
    blocks; Jacobi, GS, SGS, ILU, IC, TNS only).  After the solver's Build(): PrecondApply(rhs, x), Info()"""
    kind = PC_AS
    _LOCAL_KINDS = (PC_JACOBI, PC_ILU0, PC_MCSGS, PC_MCGS, PC_MCILU, PC_GS, PC_SGS, PC_IC, PC_TNS)

    def __init__(self, nb=1, overlap=0, local=None):
        super().__init__()
        self.form = -1
        self._solver = None
        self.Set(nb, overlap, local if local is not None else Jacobi())

    def Set(self, nb, overlap, local):
        if int(nb) < 1 or int(overlap) < 0:
            raise ValueError("AS: nb >= 1 and overlap >= 0")
        if getattr(local, "kind", None) not in self._LOCAL_KINDS:
            raise ValueError("AS: the local solvers are one of Jacobi, ILU, MultiColoredSGS / GS / ILU, GS, SGS, IC or TNS")
        own = dict(vars(local))
        local_params = own.pop("params", None) if isinstance(local, ILU) else None
        if own != vars(type(local)()):
            raise ValueError("AS: the local solvers are taken by kind, with its defaults; settings of the "
                             "%s object (parameters, format, descriptor) would not reach them" % type(local).__name__)
        self.local = local
        self.local_params = local_params
        self.params = (float(int(nb)), float(int(overlap)), float(local.kind))

    def SetForm(self, form):
        if int(form) not in (-1, 0, 1, 2):
            raise ValueError("AS: form is -1 (auto), 0 (stepwise), 1 (fused) or 2 (stacked)")
        self.form = int(form)

    def _configure(self, solver):
        capi.check(_lib().ramd_solver_set_precond_form(solver._h, self.form))
        if self.local_params is not None:
            capi.check(_lib().ramd_solver_set_precond_local_params(solver._h, *self.local_params))
        self._solver = solver

    def PrecondApply(self, rhs, x):
        """x = M^-1 rhs through the solver this object was built under"""
        self._solver.PrecondApply(rhs, x)

    def Info(self):
        """-> dict(form, nb, overlap, size, stacked_rows, uncovered, nnz_stacked, restricted) of the built plan"""
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_solver_precond_info(self._solver._h, out))
        keys = ("form", "nb", "overlap", "size", "stacked_rows", "uncovered", "nnz_stacked", "restricted")
        return dict(zip(keys, [int(v) for v in out]))


class RAS(AS):
    """restricted additive Schwarz: every row takes the result of the block that owns it; rows of no block are not written"""
    kind = PC_RAS


class ASPlan:
    """layout, restriction, prolongation and the direct sum on their own (ramd_as_*); the kernel tests drive this"""
    STEPWISE, FUSED, STACKED = 0, 1, 2

    def __init__(self, mat, nb, overlap, restricted=False, form=-1):
        self._h = C.c_void_p()
        self.dtype = mat.dtype
        capi.check(_lib().ramd_as_build(mat._h, int(nb), int(overlap), 1 if restricted else 0, int(form), C.byref(self._h)))

    def __del__(self):
        try:
            self.Clear()
        except Exception:
            pass

    def Clear(self):
        if self._h:
            _lib().ramd_as_destroy(self._h)
            self._h = None

    def Local(self, block):
        """-> LocalMatrix: block `block` (stepwise / fused) or, block 0 of the stacked form, the direct sum; once each"""
        from . import LocalMatrix
        h = capi.mat_t()
        capi.check(_lib().ramd_as_local(self._h, int(block), C.byref(h)))
        out = LocalMatrix(self.dtype)
        _lib().ramd_mat_destroy(out._h)
        out._h = h
        return out

    @staticmethod
    def _arr(vs):
        return (capi.vec_t * len(vs))(*[v._h for v in vs])

    def Split(self, rhs, r):
        capi.check(_lib().ramd_as_split(self._h, rhs._h, r._h))

    def SplitV(self, rhs, pieces):
        capi.check(_lib().ramd_as_split_v(self._h, rhs._h, self._arr(pieces), len(pieces)))

    def Join(self, z, x):
        capi.check(_lib().ramd_as_join(self._h, z._h, x._h))

    def JoinV(self, pieces, x):
        capi.check(_lib().ramd_as_join_v(self._h, self._arr(pieces), len(pieces), x._h))

    def Weights(self, w):
        capi.check(_lib().ramd_as_weights(self._h, w._h))

    def Info(self):
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_as_info(self._h, out))
        keys = ("form", "nb", "overlap", "size", "stacked_rows", "uncovered", "nnz_stacked", "restricted")
        return dict(zip(keys, [int(v) for v in out]))


class BlockPreconditioner(_Precond):
    """block preconditioner (preconditioner_blockprecond.cpp): the operator in len(sizes) x len(sizes) blocks of sizes[b]
    rows, a solver `local` on every diagonal block and a block forward substitution over the strictly lower blocks
    (diagonal=True: SetDiagonalSolver(), the diagonal blocks alone).  perm: SetPermutation, an integer array or a
    LocalVector(int32) of the operator's length -- the blocks are those of the permuted operator.  `local` is taken by its
    kind as AS takes it.  SetForm: -1 the library's choice, 0 stepwise (the reference's calls), 1 fused (one launch per
    block row and one for the solution).  After the solver's Build(): PrecondApply(rhs, x), Info()"""
    kind = PC_BLOCK
    _LOCAL_KINDS = AS._LOCAL_KINDS

    def __init__(self, sizes, local=None, diagonal=False, perm=None):
        super().__init__()
        self.form = -1
        self._solver = None
        self._perm_vec = None
        self.Set(sizes, local if local is not None else Jacobi())
        self.diagonal = bool(diagonal)
        self.SetPermutation(perm)

    def Set(self, sizes, local):
        sizes = [int(s) for s in sizes]
        if len(sizes) < 1 or any(s < 1 for s in sizes):
            raise ValueError("BlockPreconditioner: at least one block, every block with at least one row")
        if getattr(local, "kind", None) not in self._LOCAL_KINDS:
            raise ValueError("BlockPreconditioner: the block solvers are one of Jacobi, ILU, MultiColoredSGS / GS / ILU, GS, SGS, "
                             "IC or TNS")
        own = dict(vars(local))
        local_params = own.pop("params", None) if isinstance(local, ILU) else None
        if own != vars(type(local)()):
            raise ValueError("BlockPreconditioner: the block solvers are taken by kind, with its defaults; settings of the "
                             "%s object (parameters, format, descriptor) would not reach them" % type(local).__name__)
        self.sizes = sizes
        self.local = local
        self.local_params = local_params

    def SetDiagonalSolver(self):
        self.diagonal = True

    def SetLSolver(self):
        self.diagonal = False

    def SetPermutation(self, perm):
        if perm is not None and not hasattr(perm, "_h"):
            perm = np.asarray(perm)
            if perm.ndim != 1 or perm.dtype.kind not in "iu" or len(perm) != sum(self.sizes):
                raise ValueError("BlockPreconditioner: the permutation is an integer array of the operator's length")
            if not np.array_equal(np.sort(perm), np.arange(len(perm))):
                raise ValueError("BlockPreconditioner: the permutation vector is not a permutation of 0 .. n - 1")
            perm = perm.astype(np.int32)
        self.perm = perm

    def SetForm(self, form):
        if int(form) not in (-1, 0, 1):
            raise ValueError("BlockPreconditioner: form is -1 (auto), 0 (stepwise) or 1 (fused)")
        self.form = int(form)

    @property
    def params(self):
        return (1.0 if self.diagonal else 0.0, 0.0, float(self.local.kind))

    def _configure(self, solver):
        lib = _lib()
        capi.check(lib.ramd_solver_set_precond_blocks(solver._h, (C.c_int * len(self.sizes))(*self.sizes), len(self.sizes)))
        if self.perm is not None:
            pv = self.perm
            if not hasattr(pv, "_h"):
                from . import LocalVector
                pv = LocalVector(np.int32, data=self.perm)
            self._perm_vec = pv
            capi.check(lib.ramd_solver_set_precond_perm(solver._h, pv._h))
        capi.check(lib.ramd_solver_set_precond_form(solver._h, self.form))
        if self.local_params is not None:
            capi.check(lib.ramd_solver_set_precond_local_params(solver._h, *self.local_params))
        self._solver = solver

    def PrecondApply(self, rhs, x):
        """x = M^-1 rhs through the solver this object was built under"""
        self._solver.PrecondApply(rhs, x)

    def Info(self):
        """-> dict(form, nb, n, nnz_lower, diagonal, permuted, largest, smallest) of the built plan"""
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_solver_precond_info(self._solver._h, out))
        return dict(zip(BPPlan.INFO_KEYS, [int(v) for v in out]))


class BPPlan:
    """the blocks, one block row of the forward substitution and the join on their own (ramd_bp_*); the kernel tests drive this"""
    STEPWISE, FUSED = 0, 1
    INFO_KEYS = ("form", "nb", "n", "nnz_lower", "diagonal", "permuted", "largest", "smallest")

    def __init__(self, mat, sizes, perm=None, diagonal=False, form=-1):
        self._h = C.c_void_p()
        self.dtype = mat.dtype
        sizes = [int(s) for s in sizes]
        arr = (C.c_int * max(len(sizes), 1))(*sizes)
        capi.check(_lib().ramd_bp_build(mat._h, len(sizes), arr, perm._h if perm is not None else None, 1 if diagonal else 0,
                                        int(form), C.byref(self._h)))

    def __del__(self):
        try:
            self.Clear()
        except Exception:
            pass

    def Clear(self):
        if self._h:
            _lib().ramd_bp_destroy(self._h)
            self._h = None

    def Local(self, block):
        """-> LocalMatrix: diagonal block `block`; once each"""
        from . import LocalMatrix
        h = capi.mat_t()
        capi.check(_lib().ramd_bp_local(self._h, int(block), C.byref(h)))
        out = LocalMatrix(self.dtype)
        _lib().ramd_mat_destroy(out._h)
        out._h = h
        return out

    @staticmethod
    def _arr(vs):
        return (capi.vec_t * max(len(vs), 1))(*[v._h for v in vs])

    def Step(self, block, rhs, pieces, r):
        """r = the block row `block` of rhs' - L z; pieces: the solution vectors of blocks 0 .. block - 1 (more are ignored)"""
        capi.check(_lib().ramd_bp_step(self._h, int(block), rhs._h, self._arr(pieces), r._h))

    def Join(self, pieces, x):
        capi.check(_lib().ramd_bp_join(self._h, self._arr(pieces), len(pieces), x._h))

    def Info(self):
        out = (C.c_int64 * 8)()
        capi.check(_lib().ramd_bp_info(self._h, out))
        return dict(zip(self.INFO_KEYS, [int(v) for v in out]))


class MultiColoredSGS(_Precond):
    kind = PC_MCSGS

    def __init__(self):
        super().__init__()
        self.decomposition = True
        self.fused_sweeps = True

    def SetDecomposition(self, decomp):
        self.decomposition = bool(decomp)

    def SetFusedSweeps(self, on):
        self.fused_sweeps = bool(on)


class MultiColoredGS(MultiColoredSGS):
    """backward colour sweeps only (preconditioner_multicolored_gs.cpp:218-288)"""
    kind = PC_MCGS


class MultiColoredILU(MultiColoredSGS):
    """ILU(0,1) of the multi-coloured matrix (preconditioner_multicolored_ilu.cpp); p > 0 is not provided"""
    kind = PC_MCILU

    def Set(self, p, q=None, level=True):
        if p != 0 or (q is not None and q != 1):
            raise ValueError("only MultiColoredILU(0,1) is provided by this backend")


class _IterativeLinearSolver:
    kind = SOLVER_CG

    def __init__(self, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self._h = None
        self._op = None
        self._precond = None
        self._init = None
        self._basis = None
        self._fused = True
        self._verbose = 0

    def __del__(self):
        try:
            if self._h:
                _lib().ramd_solver_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def SetOperator(self, op):
        self._op = op

    def SetPreconditioner(self, p):
        self._precond = p

    def Init(self, abs_tol, rel_tol, div_tol, max_iter, min_iter=0):
        self._init = (float(abs_tol), float(rel_tol), float(div_tol), int(min_iter), int(max_iter))

    def InitMaxIter(self, max_iter):
        a = self._init or (1e-15, 1e-6, 1e8, 0, 1000000)
        self._init = (a[0], a[1], a[2], a[3], int(max_iter))

    def SetFused(self, on):
        self._fused = bool(on)

    def Verbose(self, v=1):
        self._verbose = int(v)

    def _create(self):
        h = C.c_void_p()
        pk = self._precond.kind if self._precond is not None else PC_NONE
        dt = capi.F64 if self.dtype == np.float64 else capi.F32
        capi.check(_lib().ramd_solver_create(self.kind, pk, dt, C.byref(h)))
        return h

    def Build(self):
        assert self._op is not None
        if self._h:
            _lib().ramd_solver_destroy(self._h)
        self._h = self._create()
        if self._init:
            capi.check(_lib().ramd_solver_init(self._h, *self._init))
        if self._basis:
            capi.check(_lib().ramd_solver_set_basis(self._h, self._basis))
        if self._precond is not None and self._precond.precond_format is not None:
            capi.check(_lib().ramd_solver_set_precond_format(self._h, self._precond.precond_format))
        if self._precond is not None and getattr(self._precond, "decomposition", True) is False:
            capi.check(_lib().ramd_solver_set_decomposition(self._h, 0))
        if self._precond is not None and getattr(self._precond, "fused_sweeps", True) is False:
            capi.check(_lib().ramd_solver_set_fused_sweeps(self._h, 0))
        if self._precond is not None and getattr(self._precond, "descr", None) is not None:
            d = self._precond.descr
            capi.check(_lib().ramd_solver_set_tri_solver(self._h, d.alg, d.max_iter, d.tol, int(d.use_tol)))
        if self._precond is not None and getattr(self._precond, "params", None) is not None:
            capi.check(_lib().ramd_solver_set_precond_params(self._h, *self._precond.params))
        if self._precond is not None and hasattr(self._precond, "_configure"):
            self._precond._configure(self)
        capi.check(_lib().ramd_solver_set_fused(self._h, int(self._fused)))
        capi.check(_lib().ramd_solver_set_verbose(self._h, self._verbose))
        self._configure_extra()
        capi.check(_lib().ramd_solver_build(self._h, self._op._h))

    def _configure_extra(self):
        pass

    def Solve(self, rhs, x):
        capi.check(_lib().ramd_solver_solve(self._h, rhs._h, x._h))

    def PrecondApply(self, rhs, x):
        capi.check(_lib().ramd_solver_precond_apply(self._h, rhs._h, x._h))

    def ReBuildNumeric(self):
        capi.check(_lib().ramd_solver_rebuild_numeric(self._h))

    def Clear(self):
        if self._h:
            capi.check(_lib().ramd_solver_clear(self._h))

    def _result(self):
        it, st, res = C.c_int(0), C.c_int(0), C.c_double(0)
        capi.check(_lib().ramd_solver_result(self._h, C.byref(it), C.byref(st), C.byref(res)))
        return it.value, st.value, res.value

    def GetIterationCount(self):
        return self._result()[0]

    def SetTimeMark(self, iteration):
        """measurement hook: note the wall clock (device drained) when iteration `iteration` has been checked"""
        capi.check(_lib().ramd_solver_set_time_mark(self._h, int(iteration)))

    def GetSecondsSinceTimeMark(self):
        s = C.c_double(0)
        capi.check(_lib().ramd_solver_seconds_since_time_mark(self._h, C.byref(s)))
        return s.value

    def GetSolverStatus(self):
        return self._result()[1]

    def GetCurrentResidual(self):
        return self._result()[2]

    def GetNumColors(self):
        n = C.c_int(0)
        capi.check(_lib().ramd_solver_num_colors(self._h, C.byref(n)))
        return n.value

    def GetResidualHistory(self):
        n = C.c_int(0)
        capi.check(_lib().ramd_solver_history(self._h, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), dtype=np.float64)
        capi.check(_lib().ramd_solver_history(self._h, buf.ctypes.data_as(C.POINTER(C.c_double)), n.value,
                                              C.byref(n)))
        return buf[:n.value]


class CG(_IterativeLinearSolver):
    kind = SOLVER_CG


class GMRES(_IterativeLinearSolver):
    kind = SOLVER_GMRES

    def SetBasisSize(self, m):
        self._basis = int(m)


class BiCGStab(_IterativeLinearSolver):
    kind = SOLVER_BICGSTAB


class FCG(_IterativeLinearSolver):
    """flexible CG (src/solvers/krylov/fcg.cpp)"""
    kind = SOLVER_FCG


class CR(_IterativeLinearSolver):
    """conjugate residual (src/solvers/krylov/cr.cpp)"""
    kind = SOLVER_CR


class FGMRES(GMRES):
    """flexible GMRES (src/solvers/krylov/fgmres.cpp)"""
    kind = SOLVER_FGMRES


class BiCGStabl(_IterativeLinearSolver):
    """BiCGStab(l) (src/solvers/krylov/bicgstabl.cpp), l = 2 unless SetOrder is called"""
    kind = SOLVER_BICGSTABL

    def SetOrder(self, l):
        self._basis = int(l)


class IDR(_IterativeLinearSolver):
    """IDR(s) (src/solvers/krylov/idr.cpp); s = 4 and seed = time() unless set"""
    kind = SOLVER_IDR

    def __init__(self, dtype=np.float64):
        super().__init__(dtype)
        self._seed = None

    def SetShadowSpace(self, s):
        self._basis = int(s)

    def SetRandomSeed(self, seed):
        self._seed = int(seed)

    def _configure_extra(self):
        if self._seed is not None:
            capi.check(_lib().ramd_solver_set_seed(self._h, self._seed))


class FixedPoint(_IterativeLinearSolver):
    """x += omega M^-1 (b - A x) (src/solvers/solver.cpp:517-775); needs a preconditioner"""
    kind = SOLVER_FIXEDPOINT

    def __init__(self, dtype=np.float64):
        super().__init__(dtype)
        self._omega, self._smoother = 1.0, False

    def SetRelaxation(self, omega):
        self._omega = float(omega)

    def FlagSmoother(self):
        self._smoother = True

    def _configure_extra(self):
        capi.check(_lib().ramd_solver_set_params(self._h, self._omega, 1.0 if self._smoother else 0.0))


class Chebyshev(_IterativeLinearSolver):
    """Chebyshev iteration (src/solvers/chebyshev.cpp); Set(lambda_min, lambda_max) is mandatory: the bounds of the
    spectrum of A, or of M^-1 A with a preconditioner.  Solve() without them is an error status"""
    kind = SOLVER_CHEBYSHEV

    def __init__(self, dtype=np.float64):
        super().__init__(dtype)
        self._bounds = None

    def Set(self, lambda_min, lambda_max):
        self._bounds = (float(lambda_min), float(lambda_max))

    def _configure_extra(self):
        if self._bounds is not None:
            capi.check(_lib().ramd_solver_set_params(self._h, *self._bounds))


class QMRCGStab(_IterativeLinearSolver):
    """QMRCGStab (src/solvers/krylov/qmrcgstab.cpp)"""
    kind = SOLVER_QMRCGSTAB


class MixedPrecisionDC(_IterativeLinearSolver):
    """MixedPrecisionDC<fp64, fp32>: Set(inner) takes a float32 CG/GMRES/BiCGStab object whose
    preconditioner and Init() settings are applied to the inner solver."""

    def __init__(self):
        super().__init__(np.float64)
        self._inner = None

    def Set(self, inner):
        self._inner = inner

    def _create(self):
        h = C.c_void_p()
        pk = self._inner._precond.kind if self._inner._precond is not None else PC_NONE
        capi.check(_lib().ramd_solver_create_mixed(self._inner.kind, pk, C.byref(h)))
        return h

    def _configure_extra(self):
        if self._inner._init:
            a = self._inner._init
            capi.check(_lib().ramd_solver_init_inner(self._h, a[0], a[1], a[2], a[4]))
        if self._inner._basis:
            capi.check(_lib().ramd_solver_set_basis(self._h, self._inner._basis))
        capi.check(_lib().ramd_solver_set_fused(self._h, int(self._inner._fused)))
