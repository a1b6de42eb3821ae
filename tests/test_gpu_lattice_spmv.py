"""Lattice form of the value-pattern CSR product (spmv.hip: csr_analyse_lattice; spmv_lattice.hip: k_csr_lat): a matrix whose
dictionary is that of a 5- / 7-point operator on an nx x ny x nz lattice (64 | nx) has Apply and the product with a fused dot
run on (x, y) tiles marched along z.  Everything is compared BIT FOR BIT with the CPU oracle; the fused dot to the bounds of
test_gpu_value_patterns.py (rel 1e-13 / 1e-6 of <x, y> for the definite operators, the bound of a double-precision sum of
nrow terms where the dot runs against another vector).

RAMD_CSR_LAT is read once per process, so every case runs in a fresh interpreter with RAMD_CSR_PAT=1 RAMD_CSR_PATV=1
RAMD_CSR_LAT=2 (the matrices are far below the size thresholds).  Shapes: 64 x 3 x 2 (one tile, fewer planes than a run, every
boundary pattern), 128 x 5 x 3 (the ring cell in x is the previous line's end, ny no multiple of the tile height),
192 x 17 x 4 (partial tiles in x and y), 64 x 4 x 70 (more planes than a run: the seam and its planes read twice)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

PRELUDE = r"""
import sys, ctypes as C, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import rocalution_amd as ra
from rocalution_amd import capi, generators as gen, solvers as S
from oracle import oracle
oracle.build(); oracle.set_threads(1); lib = capi.load(); ra.init_rocalution()
dtype = np.%s
TOL = %r
POISSON = [-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0]
# seven different coefficients (a swapped slot shows), diagonally dominant: x^T A x has no cancellation
SEVEN = [-0.5, -0.75, -0.875, 6.5, -1.0, -1.125, -1.25]
def lat(nx, ny, nz, coef, offs=None):
    # rows in ascending columns; a neighbour the lattice lacks is left out
    n = nx * ny * nz; r = np.arange(n, dtype=np.int64); gx = r %% nx; gy = (r // nx) %% ny; gz = r // (nx * ny)
    if offs is None:
        offs = [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
        have = [gz > 0, gy > 0, gx > 0, r >= 0, gx < nx - 1, gy < ny - 1, gz < nz - 1]
    else:
        have = [(r + o >= 0) & (r + o < n) for o in offs]
    cols = np.stack([r + o for o in offs], 1); have = np.stack(have, 1)
    vals = np.broadcast_to(np.asarray(coef, dtype=np.float64), cols.shape)
    rp = np.concatenate([[0], np.cumsum(have.sum(1))]).astype(np.int32)
    return rp, cols[have].astype(np.int32), np.ascontiguousarray(vals[have])
def eq(a, b):
    a = np.asarray(a); b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "max |diff| = %%r" %% float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))
def vec(a):
    return ra.LocalVector(dtype, data=np.ascontiguousarray(a, dtype=dtype))
def mat(rp, ci, va):
    A = ra.LocalMatrix(dtype); A.SetDataPtrCSR(rp, ci, np.ascontiguousarray(va, dtype=dtype)); return A
def apply(A, xh):
    y = ra.LocalVector(dtype); y.Allocate("", A.GetM()); A.Apply(vec(xh), y); return y.numpy()
def rnd(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
def fetch(slot):
    out = (C.c_double * 1)(); capi.check(lib.ramd_scalars_fetch(out, slot, 1)); return out[0]
def products(rp, ci, va, A, strict=True):
    # Apply and the two fused dots (k_csr_lat where the matrix is a lattice operator); ApplyAdd and the Jacobi sweep (k_csr_patv)
    va = np.ascontiguousarray(va, dtype=dtype); nrow = len(rp) - 1
    xh, y0, rhs, wh = rnd(5, nrow), rnd(6, nrow), rnd(7, nrow), rnd(9, nrow)
    ref = oracle.csr_apply(rp, ci, va, xh)
    eq(apply(A, xh), ref)
    sumabs = lambda u: nrow * 2.0 ** -53 * float(np.sum(np.abs(u.astype(np.float64) * ref.astype(np.float64))))
    w = ra.LocalVector(dtype); w.Allocate("", nrow); xv = vec(xh)
    capi.check(lib.ramd_fused_apply_dot(A._h, xv._h, w._h, 11))
    eq(w.numpy(), ref)
    got, want = fetch(11), float(np.dot(xh.astype(np.float64), ref.astype(np.float64)))
    bound = TOL * abs(want) if strict else sumabs(xh)
    assert abs(got - want) <= bound, (got, want, bound)
    w.Zeros(); wv = vec(wh)
    capi.check(lib.ramd_fused_apply_dotv(A._h, xv._h, w._h, wv._h, 12))
    eq(w.numpy(), ref)
    got, want = fetch(12), float(np.dot(wh.astype(np.float64), ref.astype(np.float64)))
    assert abs(got - want) <= sumabs(wh), (got, want, sumabs(wh))
    ya = vec(y0); A.ApplyAdd(xv, 0.375, ya)
    eq(ya.numpy(), oracle.csr_apply_add(rp, ci, va, xh, dtype(0.375), y0))
    dinv = rnd(8, nrow); omega = dtype(0.8)
    xn = ra.LocalVector(dtype); xn.Allocate("", nrow); dv, rv = vec(dinv), vec(rhs)
    capi.check(lib.ramd_fused_jacobi_sweep(A._h, dv._h, rv._h, xv._h, xn._h, float(omega)))
    t = dtype(-1) * ref + rhs; t = dinv * t
    eq(xn.numpy(), xh + omega * t)
"""

TOL = {np.float64: 1e-13, np.float32: 1e-6}
SHAPES = [(64, 3, 2), (128, 5, 3), (192, 17, 4), (64, 4, 70)]


def _run(body, dtype, env=None, timeout=300):
    code = PRELUDE % (ROOT, HERE, np.dtype(dtype).name, TOL[dtype]) + body + "\nprint('OK')\n"
    e = dict(os.environ, RAMD_CSR_PAT="1", RAMD_CSR_PATV="1", RAMD_CSR_LAT="2")
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stdout.decode()[-3000:]
    return r.stdout.decode()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_lattice_products(dtype, shape):
    """every form of the product on both coefficient sets, the lattice recognised with its dimensions"""
    _run(r"""
nx, ny, nz = %r
for coef in (POISSON, SEVEN):
    rp, ci, va = lat(nx, ny, nz, coef)
    A = mat(rp, ci, va)
    assert A.LatticeState() == 0
    products(rp, ci, va, A)
    assert A.ValuePatternState() == 1 and A.LatticeState(dims=True) == (1, (nx, ny, nz)), A.LatticeState(dims=True)
""" % (shape,), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice_device_generator(dtype):
    """GenPoisson7(64) is the host-built operator on 64 x 64 x 64"""
    _run(r"""
rp, ci, va = lat(64, 64, 64, POISSON)
n = len(rp) - 1
B = ra.LocalMatrix(dtype); B.GenPoisson7(64)
eq(apply(B, rnd(2, n)), oracle.csr_apply(rp, ci, va.astype(dtype), rnd(2, n)))
assert B.LatticeState(dims=True) == (1, (64, 64, 64)), B.LatticeState(dims=True)
products(rp, ci, va, B)
""", dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice_masking(dtype):
    """NaN and inf in x at cells that are no columns of the rows compared: the linear ring of a boundary row reads them, a slot
    the row does not have contributes no term"""
    _run(r"""
nx, ny, nz = 128, 5, 3
rp, ci, va = lat(nx, ny, nz, SEVEN)
n = len(rp) - 1
rng = np.random.default_rng(17)
bad = np.zeros(n, dtype=bool); bad[rng.choice(n, n // 20, replace=False)] = True
bad[(0 * ny + 1) * nx + nx - 1] = True       # the end of line (1, 0): the cell left of row (0, 2, 0)
bad[(2 * ny + 3) * nx] = True                # the start of line (3, 2): the cell right of row (nx - 1, 2, 2)
xh = rnd(3, n); k = np.nonzero(bad)[0]
xh[k[0::3]] = np.nan; xh[k[1::3]] = np.inf; xh[k[2::3]] = -np.inf
touched = np.add.reduceat(bad[ci].astype(np.int64), rp[:-1]) > 0     # rows with a poisoned column
keep = ~touched
r = np.arange(n); gx = r % nx; gy = (r // nx) % ny; gz = r // (nx * ny)
def reads(cond, o):          # kept rows without that neighbour whose linear cell r + o is poisoned
    idx = r[cond & keep] + o
    idx = idx[(idx >= 0) & (idx < n)]
    return int(np.count_nonzero(bad[idx]))
kinds = [reads(gx == 0, -1), reads(gx == nx - 1, 1), reads((gy == 0) & (gz > 0), -nx), reads((gy == ny - 1) & (gz < nz - 1), nx)]
assert min(kinds) > 0, kinds
A = mat(rp, ci, va)
ref = oracle.csr_apply(rp, ci, va.astype(dtype), xh)
assert np.all(np.isfinite(ref[keep]))
eq(apply(A, xh)[keep], ref[keep])
assert A.LatticeState() == 1
w = ra.LocalVector(dtype); w.Allocate("", n); xv = vec(xh)
capi.check(lib.ramd_fused_apply_dot(A._h, xv._h, w._h, 11))
eq(w.numpy()[keep], ref[keep])
""", dtype)


def test_lattice_same_bits_as_value_pattern_kernel(tmp_path):
    """y and the fetched dot slots are byte-identical between k_csr_lat (RAMD_CSR_LAT=2) and k_csr_patv (RAMD_CSR_LAT=0)"""
    outs = []
    for v in ("2", "0"):
        f = str(tmp_path / ("lat_%s.npz" % v))
        _run(r"""
rp, ci, va = lat(192, 17, 4, SEVEN)
n = len(rp) - 1
A = mat(rp, ci, va); xv = vec(rnd(5, n)); wv = vec(rnd(9, n))
y = ra.LocalVector(dtype); y.Allocate("", n); A.Apply(xv, y)
y1 = ra.LocalVector(dtype); y1.Allocate("", n); capi.check(lib.ramd_fused_apply_dot(A._h, xv._h, y1._h, 11))
y2 = ra.LocalVector(dtype); y2.Allocate("", n); capi.check(lib.ramd_fused_apply_dotv(A._h, xv._h, y2._h, wv._h, 12))
assert A.ValuePatternState() == 1 and A.LatticeState() == %d, A.LatticeState()
np.savez(%r, y=y.numpy(), y1=y1.numpy(), y2=y2.numpy(), dots=np.array([fetch(11), fetch(12)]))
""" % (1 if v == "2" else 0, f), np.float64, env={"RAMD_CSR_LAT": v})
        outs.append(dict(np.load(f)))
    for k in ("y", "y1", "y2", "dots"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice_not_eligible(dtype):
    """matrices that are no such operator: state -1, the oracle's bits from the kernels they had"""
    _run(r"""
from conftest import load_golden
def check(rp, ci, va, vstate, strict=True):
    A = mat(rp, ci, va)
    products(rp, ci, va, A, strict=strict)
    assert A.ValuePatternState() == vstate and A.LatticeState() == -1, (A.ValuePatternState(), A.LatticeState())
check(*lat(48, 4, 4, POISSON), 1)                                  # nx no multiple of 64
rp, ci, va = lat(64, 64, 1, POISSON); check(rp, ci, va, 1)         # 5-point operator in 2-D: no second distance
g = load_golden("lap27_6"); check(g["rowptr"], g["col"], g["val"], 1)
rp, ci, va = lat(64, 4, 4, POISSON); vb = va.copy(); vb[rp[300] + 1] = -1.5
check(rp, ci, vb, -1, strict=False)                                # one other value: the value state is -1 already
nx, ny, nz = 64, 4, 4                                              # an offset outside the set: +2 in every row that has it
check(*lat(nx, ny, nz, [-1.0, -1.0, -1.0, 7.0, -1.0, -0.5, -1.0, -1.0], offs=[-nx * ny, -nx, -1, 0, 1, 2, nx, nx * ny]), 1)
""", dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lattice_invalidation(dtype):
    """Scale: the state returns to 0 and the next product is the oracle's on the new values, in the lattice form again"""
    _run(r"""
rp, ci, va = lat(128, 5, 3, SEVEN)
va = va.astype(dtype); n = len(rp) - 1; xh = rnd(1, n)
A = mat(rp, ci, va)
eq(apply(A, xh), oracle.csr_apply(rp, ci, va, xh)); assert A.LatticeState() == 1
A.Scale(0.75)
assert A.ValuePatternState() == 0 and A.LatticeState() == 0, (A.ValuePatternState(), A.LatticeState())
eq(apply(A, xh), oracle.csr_apply(rp, ci, va * dtype(0.75), xh))
assert A.LatticeState() == 1
A.UseRowPatterns(False)                                            # switched off together with the dictionaries
eq(apply(A, xh), oracle.csr_apply(rp, ci, va * dtype(0.75), xh))
""", dtype)


def test_lattice_cg_jacobi(tmp_path):
    """CG + Jacobi, 30 iterations on 64 x 8 x 8: against the oracle within the CG tolerances of test_gpu_solvers.py (iterations
    +-2, history rel 1e-6 with the round-off floor, x rel 1e-6), and x byte-identical between RAMD_CSR_LAT=2 and =0"""
    outs = []
    for v in ("2", "0"):
        f = str(tmp_path / ("cg_%s.npz" % v))
        _run(r"""
rp, ci, va = lat(64, 8, 8, POISSON)
n = len(rp) - 1
b = oracle.csr_apply(rp, ci, va, np.ones(n))
A = mat(rp, ci, va)
x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Init(0.0, 0.0, 1e300, 30); ls.Build()
ls.Solve(vec(b), x)
assert A.LatticeState() == %d, A.LatticeState()
ref = oracle.solve(rp, ci, va, b, solver=oracle.CG, precond=oracle.PC_JACOBI, abs_tol=0.0, rel_tol=0.0, div_tol=1e300, max_iter=30)
assert abs(ls.GetIterationCount() - ref["iters"]) <= 2, (ls.GetIterationCount(), ref["iters"])
h, r = np.asarray(ls.GetResidualHistory()), np.asarray(ref["history"])
m = min(len(h), len(r)) - 2
assert m >= 25, m
assert np.all(np.abs(h[:m] - r[:m]) <= 1e-6 * np.abs(r[:m]) + 1e-12 * h[0]), np.max(np.abs(h[:m] / r[:m] - 1))
assert np.linalg.norm(x.numpy() - ref["x"]) / np.linalg.norm(ref["x"]) < 1e-6
np.savez(%r, hist=h, x=x.numpy())
""" % (1 if v == "2" else 0, f), np.float64, env={"RAMD_CSR_LAT": v})
        outs.append(dict(np.load(f)))
    for k in ("hist", "x"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
