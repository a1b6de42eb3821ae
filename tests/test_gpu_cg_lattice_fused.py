"""CG + Jacobi on a lattice operator: the direction update of one iteration and the product of the next as ONE launch
(spmv_lattice.hip: k_cg_lat; fused.hip: ramd_fused_cg_direction_apply_dot and its _ready query; solvers.hpp: CG::doFusedLoop).

Every expected value comes from the pair the launch replaces -- ramd_fused_cg_direction_dc, then ramd_fused_apply_dot -- run
on copies of the same inputs, and is compared without a tolerance: vectors as bytes, the <p, q> slot as bits.  Whole solves
are compared between RAMD_CG_LATDIR unset and =0.

RAMD_CSR_LAT and RAMD_CG_LATDIR are read once per process, so every case runs in a fresh interpreter with RAMD_CSR_PAT=1
RAMD_CSR_PATV=1 RAMD_CSR_LAT=2.  Shapes: those of test_gpu_lattice_spmv.py -- 64 x 3 x 2 (one half-empty tile, fewer planes than
a run), 128 x 5 x 3 (the ring cell in x is the previous line's end), 192 x 17 x 4 (partial tiles in x and y and several tiles:
a p updated in place would show), 64 x 4 x 70 (more planes than a run: seam planes are formed twice by different workgroups)
-- and 256 x 9 x 17 (two tiles side by side in x, a one-plane second run)."""
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
lib = capi.load(); ra.init_rocalution()
dtype = np.%s
POISSON = [-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0]
SEVEN = [-0.5, -0.75, -0.875, 6.5, -1.0, -1.125, -1.25]
S_PQ, S_RHO, S_RR, S_NEW = 0, 1, 2, 3          # slots as CG lays them out
RHO, PQ, NEW = 0.731, -1.917, 0.377            # (no dyadic values: every coefficient is rounded in the vectors' type)
def lat(nx, ny, nz, coef):
    # rows in ascending columns; a neighbour the lattice lacks is left out
    n = nx * ny * nz; r = np.arange(n, dtype=np.int64); gx = r %% nx; gy = (r // nx) %% ny; gz = r // (nx * ny)
    offs = [-nx * ny, -nx, -1, 0, 1, nx, nx * ny]
    have = [gz > 0, gy > 0, gx > 0, r >= 0, gx < nx - 1, gy < ny - 1, gz < nz - 1]
    cols = np.stack([r + o for o in offs], 1); have = np.stack(have, 1)
    vals = np.broadcast_to(np.asarray(coef, dtype=np.float64), cols.shape)
    rp = np.concatenate([[0], np.cumsum(have.sum(1))]).astype(np.int32)
    return rp, cols[have].astype(np.int32), np.ascontiguousarray(vals[have])
def same(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        bad = np.flatnonzero(a.view(u) != b.view(u))
        raise AssertionError("%%s: %%d of %%d elements differ, first at %%d: %%r != %%r" %% (what, len(bad), a.size, bad[0], a[bad[0]], b[bad[0]]))
def vec(a, dt=None):
    dt = dt or dtype
    return ra.LocalVector(dt, data=np.ascontiguousarray(a, dtype=dt))
def mat(rp, ci, va, dt=None):
    dt = dt or dtype
    A = ra.LocalMatrix(dt); A.SetDataPtrCSR(rp, ci, np.ascontiguousarray(va, dtype=dt)); return A
def rnd(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(dtype)
def setslots():
    for s, v in ((S_RHO, RHO), (S_PQ, PQ), (S_RR, -7.0), (S_NEW, NEW)):
        capi.check(lib.ramd_scalars_set(s, float(v)))
def slotbits(slot):
    out = (C.c_double * 1)(); capi.check(lib.ramd_scalars_fetch(out, slot, 1)); return np.array([out[0]]).view(np.uint64)[0]
def form(v):
    h = C.c_void_p(); capi.check(lib.ramd_dcode_create_from_vector(v._h, C.byref(h))); return h
def forminfo(h):
    kind, count = C.c_int(-1), C.c_int(-1); capi.check(lib.ramd_dcode_info(h, C.byref(kind), C.byref(count), None)); return kind.value, count.value
def dinvs(n):
    # the three inverse diagonals: one value (uniform); three values placed irregularly; 256 distinct values, all present
    rng = np.random.default_rng(11)
    three = np.array([1.0 / 6.0, 1.0 / 12.0, 0.37], dtype)
    many = (0.05 + np.arange(256) / 300.0).astype(dtype)
    return {"uniform": (np.full(n, 1.0 / 6.0, dtype), (1, 1)), "three": (three[rng.integers(0, 3, n)], (2, 3)),
            "many": (np.concatenate([many, rng.choice(many, n - 256)]), (2, 256))}
def ready(A, h):
    yes = C.c_int(-1); capi.check(lib.ramd_fused_cg_direction_apply_dot_ready(A._h, h, C.byref(yes))); return yes.value
def pair(A, h, x0, p0, r0):
    # the two launches the fused one replaces, on copies -> x, p, q, bits of <p, q>
    n = len(x0); x, p, r = vec(x0), vec(p0), vec(r0); q = vec(np.full(n, -3.0))
    setslots()
    capi.check(lib.ramd_fused_cg_direction_dc(x._h, p._h, r._h, h, S_RHO, S_PQ, S_NEW))
    capi.check(lib.ramd_fused_apply_dot(A._h, p._h, q._h, S_PQ))
    same(r.numpy(), r0, "the pair reads r only")
    return x.numpy(), p.numpy(), q.numpy(), slotbits(S_PQ)
def fused(A, h, x0, p0, r0):
    n = len(x0); x, po, r = vec(x0), vec(p0), vec(r0); pn, q = vec(np.full(n, -5.0)), vec(np.full(n, -3.0))
    setslots()
    capi.check(lib.ramd_fused_cg_direction_apply_dot(A._h, x._h, po._h, pn._h, r._h, q._h, h, S_RHO, S_PQ, S_NEW))
    got = x.numpy(), pn.numpy(), q.numpy(), slotbits(S_PQ)
    same(po.numpy(), p0, "p_old is only read"); same(r.numpy(), r0, "r is only read")
    return got
def compare(A, h, x0, p0, r0, what):
    want = pair(A, h, x0, p0, r0)          # (also runs the analyses of the matrix)
    assert A.LatticeState() == 1 and ready(A, h) == 1, (what, A.LatticeState(), ready(A, h))
    got = fused(A, h, x0, p0, r0)
    for name, a, b in zip(("x", "p_new", "q"), got[:3], want[:3]):
        same(a, b, "%%s %%s" %% (what, name))
    print(what, "<p,q> bits", hex(got[3]), hex(want[3]))
    assert got[3] == want[3], (what, got[3], want[3])
"""

SHAPES = [(64, 3, 2), (128, 5, 3), (192, 17, 4), (64, 4, 70), (256, 9, 17)]
DTYPES = [np.float64, np.float32]
_ids = lambda s: "%dx%dx%d" % s


def _run(body, dtype=np.float64, env=None, timeout=300):
    code = PRELUDE % (ROOT, HERE, np.dtype(dtype).name) + body + "\nprint('OK')\n"
    e = dict(os.environ, RAMD_CSR_PAT="1", RAMD_CSR_PATV="1", RAMD_CSR_LAT="2")
    e.pop("RAMD_CG_LATDIR", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stdout.decode()[-3000:]
    return r.stdout.decode()


# ================================================================ 1: the launch against the pair it replaces
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_launch_equals_the_pair(dtype, shape):
    """x, p_new, q and the <p, q> slot byte for byte, p_old and r untouched: both coefficient sets, a uniform inverse diagonal
    and coded ones of 3 and of 256 values"""
    _run(r"""
nx, ny, nz = %r
n = nx * ny * nz
for ci_, coef in enumerate((POISSON, SEVEN)):
    A = mat(*lat(nx, ny, nz, coef))
    for name, (d, info) in dinvs(n).items():
        h = form(vec(d)); assert forminfo(h) == info, (name, forminfo(h))
        compare(A, h, rnd(21 + ci_, n), rnd(22 + ci_, n), rnd(23 + ci_, n), "%%s %%s" %% ("poisson seven".split()[ci_], name))
        capi.check(lib.ramd_dcode_destroy(h))
""" % (shape,), dtype)


# ================================================================ 2: special values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(192, 17, 4), (64, 4, 70), (256, 9, 17)], ids=_ids)
def test_special_values(dtype, shape):
    """NaN, +-inf and -0.0 in p_old and r at tile corners, in ring positions (the cells around a 128 x 8 tile), on seam planes
    (the last plane of a run and the first of the next) and in the first and last row: every output equals the pair's"""
    _run(r"""
nx, ny, nz = %r
n = nx * ny * nz
TX, TY = 128, 8
# (a lattice this small has fewer tiles than the workgroups wanted: runs of 16 planes)
zs = sorted({0, nz - 1} | {z for z in (15, 16, 17, 31, 32, 63, 64) if z < nz})
ys = sorted({y for y in (0, TY - 1, TY, TY + 1, 2 * TY - 1, 2 * TY, ny - 1) if 0 <= y < ny})
xs = sorted({x for x in (0, 1, 63, 64, TX - 1, TX, TX + 1, nx - 1) if 0 <= x < nx})
cells = [(z * ny + y) * nx + x for z in zs for y in ys for x in xs] + [0, n - 1]
specials = [np.nan, np.inf, -np.inf, -0.0]
A = mat(*lat(nx, ny, nz, SEVEN))
for name in ("uniform", "three"):
    d, info = dinvs(n)[name]
    h = form(vec(d))
    x0, p0, r0 = rnd(31, n), rnd(32, n), rnd(33, n)
    for k, c in enumerate(cells):               # p and r take turns, every fourth cell gets both
        if k %% 4 != 1:
            p0[c] = specials[k %% 4]
        if k %% 4 != 0:
            r0[c] = specials[(k // 4) %% 4]
    assert np.isnan(p0).any() and np.isinf(r0).any() and np.signbit(p0[p0 == 0]).any()
    compare(A, h, x0, p0, r0, "specials " + name)
    capi.check(lib.ramd_dcode_destroy(h))
""" % (shape,), dtype)


# ================================================================ 3: whole solves
SOLVE = r"""
nx, ny, nz = %r
rp, ci, va = lat(nx, ny, nz, POISSON)
n = len(rp) - 1
b = oracle.csr_apply(rp, ci, va, np.ones(n))
A = mat(rp, ci, va)
x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
ls = S.CG(dtype); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Init(*%r); ls.Build()
rhs = vec(b)
ls.Solve(rhs, x)
out = dict(x=x.numpy(), it=np.array([ls.GetIterationCount()]), hist=np.asarray(ls.GetResidualHistory()))
if %r:                                        # a second Solve on the same built solver, from the iterate of the first
    ls.Solve(rhs, x)
    out.update(x2=x.numpy(), it2=np.array([ls.GetIterationCount()]), hist2=np.asarray(ls.GetResidualHistory()))
dv = ra.LocalVector(dtype); dv.Allocate("", n); A.ExtractInverseDiagonal(dv); h = form(dv)
assert A.LatticeState() == 1 and forminfo(h)[0] in (1, 2), (A.LatticeState(), forminfo(h))
assert ready(A, h) == %d, ready(A, h)
np.savez(%r, **out)
"""


def _solves(tmp_path, shape, init, dtype=np.float64, again=False):
    outs = []
    for v in (None, "0"):
        f = str(tmp_path / ("cg_%s.npz" % v))
        body = "oracle.build(); oracle.set_threads(1)\n" + SOLVE % (shape, init, again, 0 if v == "0" else 1, f)
        _run(body, dtype, env={} if v is None else {"RAMD_CG_LATDIR": v})
        outs.append(dict(np.load(f)))
    on, off = outs
    assert sorted(on) == sorted(off)
    for k in on:
        assert on[k].dtype == off[k].dtype and on[k].tobytes() == off[k].tobytes(), (k, on[k], off[k])
    return on


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_solves_identical_with_the_switch_unset_and_off(tmp_path, shape):
    """CG + Jacobi, 40 iterations: x byte-equal, iteration count and residual history equal"""
    on = _solves(tmp_path, shape, (0.0, 0.0, 1e300, 40))
    assert on["it"][0] == 40 and len(on["hist"]) >= 40, (on["it"], len(on["hist"]))


def test_solve_that_stops_by_tolerance(tmp_path):
    """the exit with the extra queued launch: the stopping rule ends the loop before max_iter"""
    on = _solves(tmp_path, (192, 17, 4), (0.0, 1e-6, 1e300, 1000))
    assert 5 < on["it"][0] < 1000, on["it"]


def test_second_solve_after_an_odd_number_of_iterations(tmp_path):
    """the buffers of p have swapped roles an odd number of times when the second Solve of the same solver starts"""
    on = _solves(tmp_path, (128, 5, 3), (0.0, 0.0, 1e300, 7), again=True)
    assert on["it"][0] == 7 and on["it2"][0] == 7, (on["it"], on["it2"])
    assert on["x2"].tobytes() != on["x"].tobytes()


def test_mixed_precision_inner_cg(tmp_path):
    """the fp32 inner CG of MixedPrecisionDC takes the path like any other CG: x, outer iterations and history equal"""
    outs = []
    for v in (None, "0"):
        f = str(tmp_path / ("mp_%s.npz" % v))
        _run(r"""
oracle.build(); oracle.set_threads(1)
rp, ci, va = lat(192, 17, 4, POISSON)
n = len(rp) - 1
b = oracle.csr_apply(rp, ci, va, np.ones(n))
A = mat(rp, ci, va)
x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
inner = S.CG(np.float32); inner.SetPreconditioner(S.Jacobi()); inner.Init(1e-5, 1e-2, 1e20, 100000)
mp = S.MixedPrecisionDC(); mp.SetOperator(A); mp.Set(inner); mp.Init(1e-10, 1e-8, 1e8, 100); mp.Build()
mp.Solve(vec(b), x)
assert mp.GetIterationCount() > 1, mp.GetIterationCount()
assert np.linalg.norm(x.numpy() - 1.0) / np.sqrt(n) < 1e-6
np.savez(%r, x=x.numpy(), it=np.array([mp.GetIterationCount()]), hist=np.asarray(mp.GetResidualHistory()))
""" % f, np.float64, env={} if v is None else {"RAMD_CG_LATDIR": v})
        outs.append(dict(np.load(f)))
    for k in ("x", "it", "hist"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


# ================================================================ 4: refusals
def test_refusals():
    """every aliasing pair, dtype and size mismatches, a matrix without lattice state 1, a missing form or one of kind none
    and bad slots: RAMD_ERR_ARG, nothing launched (the vectors and the slot keep their bytes)"""
    _run(r"""
nx, ny, nz = 128, 5, 3
n = nx * ny * nz
A = mat(*lat(nx, ny, nz, SEVEN))
d, _ = dinvs(n)["three"]
h = form(vec(d)); h32 = form(vec(d, np.float32)); hshort = form(vec(d[:n - 64]))
hnone = form(vec(np.random.default_rng(3).uniform(1, 2, n))); assert forminfo(hnone)[0] == 0
x0, p0, r0 = rnd(41, n), rnd(42, n), rnd(43, n)
compare(A, h, x0, p0, r0, "the entry works on these operands")
B = mat(*lat(nx, ny, nz, SEVEN))                 # the same operator, never applied: lattice state 0
assert B.LatticeState() == 0 and ready(B, h) == 0
vs = [vec(v) for v in (x0, p0, np.full(n, -5.0), r0, np.full(n, -3.0))]      # x, p_old, p_new, r, q
before = [v.numpy() for v in vs]
ok = (S_RHO, S_PQ, S_NEW)
setslots(); s0 = slotbits(S_PQ)
call = lambda m, w, f, sl: lib.ramd_fused_cg_direction_apply_dot(m._h, *[v._h for v in w], f, *sl)
bad = []
for i in range(5):                             # every aliasing pair
    for j in range(i + 1, 5):
        w = list(vs); w[j] = w[i]; bad.append(call(A, w, h, ok))
for k in range(5):                             # a vector of another type, of another size
    for other in (vec(np.zeros(n), np.float32), vec(np.zeros(n - 64))):
        w = list(vs); w[k] = other; bad.append(call(A, w, h, ok))
bad += [call(B, vs, h, ok)]                    # no lattice state 1
bad += [call(A, vs, f, ok) for f in (None, hnone, h32, hshort)]
for k in range(3):
    for v in (-1, 512):
        sl = list(ok); sl[k] = v; bad.append(call(A, vs, h, sl))
bad += [lib.ramd_fused_cg_direction_apply_dot(None, *[v._h for v in vs], h, *ok),
        lib.ramd_fused_cg_direction_apply_dot_ready(None, h, C.byref(C.c_int())), lib.ramd_fused_cg_direction_apply_dot_ready(A._h, h, None)]
assert len(bad) == 10 + 10 + 1 + 4 + 6 + 3 and all(s == capi.ERR_ARG for s in bad), bad
for v, w in zip(vs, before):
    same(v.numpy(), w, "refused calls leave the vectors alone")
assert slotbits(S_PQ) == s0
assert B.LatticeState() == 0
assert ready(A, None) == 0 and ready(A, hnone) == 0 and ready(A, h32) == 0 and ready(A, hshort) == 0 and ready(A, h) == 1
""")


@pytest.mark.parametrize("env", [{"RAMD_CSR_LAT": "0"}, {"RAMD_CG_LATDIR": "0"}], ids=["CSR_LAT=0", "CG_LATDIR=0"])
def test_query_says_no(env):
    """... with the lattice kernel or the fused launch switched off, and for a matrix that is no lattice operator; the entry
    refuses where the query says no"""
    _run(r"""
nx, ny, nz = 128, 5, 3
n = nx * ny * nz
A = mat(*lat(nx, ny, nz, SEVEN))
h = form(vec(dinvs(n)["uniform"][0]))
x0, p0, r0 = rnd(41, n), rnd(42, n), rnd(43, n)
pair(A, h, x0, p0, r0)
assert ready(A, h) == 0
vs = [vec(v) for v in (x0, p0, np.full(n, -5.0), r0, np.full(n, -3.0))]
assert lib.ramd_fused_cg_direction_apply_dot(A._h, *[v._h for v in vs], h, S_RHO, S_PQ, S_NEW) == capi.ERR_ARG
same(vs[2].numpy(), np.full(n, -5.0, dtype), "nothing was launched")
""", env=env)


def test_query_says_no_for_another_operator():
    _run(r"""
A = ra.LocalMatrix(dtype); A.GenLaplace27(8)
n = A.GetM()
h = form(vec(np.full(n, 0.25)))
pair(A, h, rnd(1, n), rnd(2, n), rnd(3, n))
assert A.LatticeState() == -1 and ready(A, h) == 0, A.LatticeState()
""")


# ================================================================ 5: paths that keep their three launches
@pytest.mark.parametrize("which", ["row patterns off", "27-point"])
def test_other_paths_against_the_oracle(which):
    """CG + Jacobi where the fused launch does not apply: the oracle's result within the CG tolerances of test_gpu_solvers.py
    (iterations +-2, history rel 1e-6 with the round-off floor, x rel 1e-6)"""
    _run(r"""
oracle.build(); oracle.set_threads(1)
if %r == "27-point":
    A = ra.LocalMatrix(dtype); A.GenLaplace27(8)
    rp, ci, va = gen.laplace27(8)
else:
    rp, ci, va = lat(64, 8, 8, POISSON)
    A = mat(rp, ci, va); A.UseRowPatterns(False)
n = len(rp) - 1
b = oracle.csr_apply(rp, ci, va, np.ones(n))
x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
ls = S.CG(); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Init(0.0, 0.0, 1e300, 30); ls.Build()
ls.Solve(vec(b), x)
dv = ra.LocalVector(dtype); dv.Allocate("", n); A.ExtractInverseDiagonal(dv)
assert ready(A, form(dv)) == 0
ref = oracle.solve(rp, ci, va, b, solver=oracle.CG, precond=oracle.PC_JACOBI, abs_tol=0.0, rel_tol=0.0, div_tol=1e300, max_iter=30)
assert abs(ls.GetIterationCount() - ref["iters"]) <= 2, (ls.GetIterationCount(), ref["iters"])
h, r = np.asarray(ls.GetResidualHistory()), np.asarray(ref["history"])
m = min(len(h), len(r)) - 2
assert m >= 25, m
assert np.all(np.abs(h[:m] - r[:m]) <= 1e-6 * np.abs(r[:m]) + 1e-12 * h[0]), np.max(np.abs(h[:m] / r[:m] - 1))
assert np.linalg.norm(x.numpy() - ref["x"]) / np.linalg.norm(ref["x"]) < 1e-6
""" % which)
