"""CG + Jacobi on a lattice operator: x updated by every second launch, for two iterations at once
(spmv_lattice.hip: k_cg_lat's x modes; fused.hip: ramd_fused_cg_direction_apply_dot_xpair and its _ready query; solvers.hpp:
CG::doFusedLoop).  A deferring launch leaves x alone and keeps its alpha in a slot; the next one finds the direction of the
deferring launch in the buffer it is about to store the new direction to and forms x = (x + a_prev p_prev) + alpha p.

Every expected value comes from the entries that were there before -- ramd_fused_cg_direction_apply_dot and
ramd_fused_cg_update_dc, chained as CG::doFusedLoop chains them -- run on copies of the same inputs, and is compared without a
tolerance: vectors as bytes, slots as bits.  (The one exception is the alpha a deferring launch stores: one IEEE division of
two numbers rounded to the vectors' type, formed here by numpy.)  Whole solves are compared between RAMD_CG_XPAIR unset, =0
and RAMD_CG_LATDIR=0.

The switches are read once per process, so every case runs in a fresh interpreter with RAMD_CSR_PAT=1 RAMD_CSR_PATV=1
RAMD_CSR_LAT=2.  Shapes: those of test_gpu_cg_lattice_fused.py -- 64 x 3 x 2 (one half-empty tile, fewer planes than a run),
128 x 5 x 3 (the ring cell in x is the previous line's end), 192 x 17 x 4 (partial tiles in x and y and several tiles),
64 x 4 x 70 (more planes than a run: seam planes are formed twice by different workgroups) and 256 x 9 x 17 (two tiles side by
side in x, a one-plane second run)."""
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
S_PQ, S_RHO, S_RR, S_NEW, S_ALPHA = 0, 1, 2, 3, 4          # slots as CG lays them out
RHO, PQ, NEW, STALE = 0.731, -1.917, 0.377, 123.456        # (no dyadic values: every coefficient is rounded in the vectors' type)
EACH, DEFER, BOTH = 0, 1, 2                                # (EACH: the entry that was there before)
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
    for s, v in ((S_RHO, RHO), (S_PQ, PQ), (S_RR, -7.0), (S_NEW, NEW), (S_ALPHA, STALE)):
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
def xready(A, h):
    yes = C.c_int(-1); capi.check(lib.ramd_fused_cg_direction_apply_dot_xpair_ready(A._h, h, C.byref(yes))); return yes.value
def warm(A, n):
    # the first product with a fused dot runs the analyses of the matrix
    p, q = vec(np.ones(n)), vec(np.zeros(n)); capi.check(lib.ramd_fused_apply_dot(A._h, p._h, q._h, S_PQ))
    assert A.LatticeState() == 1, A.LatticeState()
def launch(mode, A, x, po, pn, r, q, h, sr, sn):
    if mode == EACH:
        capi.check(lib.ramd_fused_cg_direction_apply_dot(A._h, x._h, po._h, pn._h, r._h, q._h, h, sr, S_PQ, sn))
    else:
        capi.check(lib.ramd_fused_cg_direction_apply_dot_xpair(A._h, x._h, po._h, pn._h, r._h, q._h, h, sr, S_PQ, sn, S_ALPHA, mode))
NAMES = ("x", "p buffer a", "p buffer b", "q", "r", "rho slot", "<p,q> slot", "<r,r> slot", "new slot")
def chain(A, h, x0, pa0, pb0, r0, modes):
    # len(modes) launches as CG::doFusedLoop queues them: the residual update between two of them, the two buffers of p and
    # the two slots of rho swapping roles after each -> the five vectors and the four slots of the loop
    n = len(x0); x, pa, pb, r = vec(x0), vec(pa0), vec(pb0), vec(r0); q = vec(np.full(n, -3.0))
    bufs = (pa, pb)
    setslots()
    sr, sn = S_RHO, S_NEW
    for k, mode in enumerate(modes):
        if k > 0:
            capi.check(lib.ramd_fused_cg_update_dc(r._h, q._h, h, sr, S_PQ, S_RR, sn))
        launch(mode, A, x, pa, pb, r, q, h, sr, sn)
        pa, pb = pb, pa; sr, sn = sn, sr
    return [x.numpy(), bufs[0].numpy(), bufs[1].numpy(), q.numpy(), r.numpy()] + [slotbits(s) for s in (S_RHO, S_PQ, S_RR, S_NEW)]
def compare_chains(A, h, x0, pa0, pb0, r0, launches, what, finite=True):
    want = chain(A, h, x0, pa0, pb0, r0, [EACH] * launches)
    got = chain(A, h, x0, pa0, pb0, r0, [DEFER, BOTH] * (launches // 2))
    if finite:                                  # (the comparison is of numbers, not of NaNs that swallowed them)
        assert all(np.isfinite(v).all() for v in want[:5]), what
    for name, a, b in zip(NAMES, got, want):
        if name.endswith("slot"):
            assert a == b, (what, name, hex(a), hex(b))
        else:
            same(a, b, "%%s, %%d launches: %%s" %% (what, launches, name))
    print(what, launches, "launches: equal; <p,q> bits", hex(got[6]))
"""

SHAPES = [(64, 3, 2), (128, 5, 3), (192, 17, 4), (64, 4, 70), (256, 9, 17)]
DTYPES = [np.float64, np.float32]
_ids = lambda s: "%dx%dx%d" % s


def _run(body, dtype=np.float64, env=None, timeout=300):
    code = PRELUDE % (ROOT, HERE, np.dtype(dtype).name) + body + "\nprint('OK')\n"
    e = dict(os.environ, RAMD_CSR_PAT="1", RAMD_CSR_PATV="1", RAMD_CSR_LAT="2")
    e.pop("RAMD_CG_LATDIR", None)
    e.pop("RAMD_CG_XPAIR", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", code], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    assert r.returncode == 0 and b"OK" in r.stdout, r.stdout.decode()[-3000:]
    return r.stdout.decode()


# ================================================================ 1: defer + both against two launches of the existing entry
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_two_and_four_iterations_equal_the_existing_entry(dtype, shape):
    """x, both buffers of p, q, r and the slots of rho, <p,q>, <r,r> and new byte for byte after two launches and after four
    (the second pair reads what the first one left): both coefficient sets, a uniform inverse diagonal and coded ones of 3
    and of 256 values"""
    _run(r"""
nx, ny, nz = %r
n = nx * ny * nz
for ci_, coef in enumerate((POISSON, SEVEN)):
    A = mat(*lat(nx, ny, nz, coef)); warm(A, n)
    for name, (d, info) in dinvs(n).items():
        h = form(vec(d)); assert forminfo(h) == info, (name, forminfo(h))
        assert ready(A, h) == 1 and xready(A, h) == 1
        what = "%%s %%s" %% ("poisson seven".split()[ci_], name)
        for launches in (2, 4):
            compare_chains(A, h, rnd(21 + ci_, n), rnd(22 + ci_, n), rnd(24 + ci_, n), rnd(23 + ci_, n), launches, what)
        capi.check(lib.ramd_dcode_destroy(h))
""" % (shape,), dtype)


# ================================================================ 2: the deferring launch alone
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_defer_alone(dtype, shape):
    """x keeps its bytes, s[slot_alpha] has the bits of (T)rho / (T)pq, p_new, q and the <p,q> slot are the existing entry's;
    p_old, r and the slots of rho and new are only read"""
    _run(r"""
nx, ny, nz = %r
n = nx * ny * nz
for ci_, coef in enumerate((POISSON, SEVEN)):
    A = mat(*lat(nx, ny, nz, coef)); warm(A, n)
    for name, (d, info) in dinvs(n).items():
        h = form(vec(d))
        x0, p0, r0 = rnd(51 + ci_, n), rnd(52 + ci_, n), rnd(53 + ci_, n)
        outs = []
        for mode in (EACH, DEFER):
            x, po, pn, r, q = vec(x0), vec(p0), vec(np.full(n, -5.0)), vec(r0), vec(np.full(n, -3.0))
            setslots()
            launch(mode, A, x, po, pn, r, q, h, S_RHO, S_NEW)
            same(po.numpy(), p0, "p_old is only read"); same(r.numpy(), r0, "r is only read")
            assert slotbits(S_RHO) == np.array([RHO]).view(np.uint64)[0] and slotbits(S_NEW) == np.array([NEW]).view(np.uint64)[0]
            outs.append((x.numpy(), pn.numpy(), q.numpy(), slotbits(S_PQ), slotbits(S_ALPHA)))
        each, defer = outs
        same(defer[0], x0, name + ": x of the deferring launch")
        assert each[0].tobytes() != x0.tobytes()
        same(defer[1], each[1], name + ": p_new"); same(defer[2], each[2], name + ": q")
        assert defer[3] == each[3], (name, hex(defer[3]), hex(each[3]))
        alpha = np.array([dtype(RHO) / dtype(PQ)]).astype(np.float64).view(np.uint64)[0]
        print(name, "alpha bits", hex(defer[4]), hex(alpha))
        assert defer[4] == alpha, (name, hex(defer[4]), hex(alpha))
        assert each[4] == np.array([STALE]).view(np.uint64)[0], "the existing entry knows no slot_alpha"
        capi.check(lib.ramd_dcode_destroy(h))
""" % (shape,), dtype)


# ================================================================ 3: special values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(192, 17, 4), (64, 4, 70), (256, 9, 17)], ids=_ids)
def test_special_values(dtype, shape):
    """NaN, +-inf and -0.0 in both buffers of p, in r and in x at tile corners, in ring positions (the cells around a
    128 x 8 tile), on seam planes (the last plane of a run and the first of the next) and in the first and last row: defer +
    both leave the bytes of two launches of the existing entry"""
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
A = mat(*lat(nx, ny, nz, SEVEN)); warm(A, n)
for name in ("uniform", "three"):
    d, info = dinvs(n)[name]
    h = form(vec(d))
    x0, pa0, pb0, r0 = rnd(31, n), rnd(32, n), rnd(34, n), rnd(33, n)
    for k, c in enumerate(cells):               # the four vectors take turns, every fourth cell gets several
        if k %% 4 != 1:
            pa0[c] = specials[k %% 4]
        if k %% 4 != 0:
            r0[c] = specials[(k // 4) %% 4]
        if k %% 3 != 1:
            x0[c] = specials[(k // 3) %% 4]
        if k %% 3 != 0:
            pb0[c] = specials[(k // 2) %% 4]
    for v in (x0, pa0, pb0, r0):
        assert np.isnan(v).any() and np.isinf(v).any() and np.signbit(v[v == 0]).any()
    compare_chains(A, h, x0, pa0, pb0, r0, 2, "specials " + name, finite=False)
    capi.check(lib.ramd_dcode_destroy(h))
""" % (shape,), dtype)


# ================================================================ 4: whole solves
# three processes per case: the switch unset, RAMD_CG_XPAIR=0, RAMD_CG_LATDIR=0.  Every solver solves twice from the same
# start, the second time with its launches counted: a Solve that left an update pending, or a solver that did not start
# its second Solve with a deferring launch, shows in x2.
SOLVE = r"""
oracle.build(); oracle.set_threads(1)
nx, ny, nz = %r
rp, ci, va = lat(nx, ny, nz, POISSON)
n = len(rp) - 1
b = oracle.csr_apply(rp, ci, va, np.ones(n))
A = mat(rp, ci, va)
rhs = vec(b)
def count(ch):
    c = C.c_int64(-1); capi.check(lib.ramd_prof_count(ch, C.byref(c))); return c.value
out = {}
for init in %r:
    tag = "_%%d" %% init[3]
    x = ra.LocalVector(dtype); x.Allocate("", n); x.Zeros()
    ls = S.CG(dtype); ls.SetOperator(A); ls.SetPreconditioner(S.Jacobi()); ls.Init(*init); ls.Build()
    ls.Solve(rhs, x)
    out.update({"x" + tag: x.numpy(), "it" + tag: np.array([ls.GetIterationCount()]), "hist" + tag: np.asarray(ls.GetResidualHistory())})
    if %r:                                    # a second Solve on the same built solver, from the iterate of the first
        ls.Solve(rhs, x)
        out.update({"xx" + tag: x.numpy(), "itt" + tag: np.array([ls.GetIterationCount()]), "histt" + tag: np.asarray(ls.GetResidualHistory())})
    x.Zeros()
    c0 = np.array([count(0), count(5)])       # (ramd_prof_count counts whether or not a channel is timed)
    ls.Solve(rhs, x)
    out.update({"x2" + tag: x.numpy(), "it2" + tag: np.array([ls.GetIterationCount()]), "launches" + tag: np.array([count(0), count(5)]) - c0})
    same(out["x2" + tag], out["x" + tag], "the same Solve again")
    ls.Clear()
dv = ra.LocalVector(dtype); dv.Allocate("", n); A.ExtractInverseDiagonal(dv); h = form(dv)
assert A.LatticeState() == 1 and forminfo(h)[0] in (1, 2), (A.LatticeState(), forminfo(h))
assert (ready(A, h), xready(A, h)) == %r, (ready(A, h), xready(A, h))
np.savez(%r, **out)
"""
VARIANTS = [("on", {}, (1, 1)), ("xpair0", {"RAMD_CG_XPAIR": "0"}, (1, 0)), ("latdir0", {"RAMD_CG_LATDIR": "0"}, (0, 0))]


def _solves(tmp_path, shape, inits, dtype=np.float64, again=False):
    outs = {}
    for name, env, answers in VARIANTS:
        f = str(tmp_path / ("cg_%s.npz" % name))
        _run(SOLVE % (shape, inits, again, answers, f), dtype, env=env)
        outs[name] = dict(np.load(f))
    on = outs["on"]
    for name in ("xpair0", "latdir0"):
        off = outs[name]
        assert sorted(on) == sorted(off)
        for k in on:
            if not k.startswith("launches"):
                assert on[k].dtype == off[k].dtype and on[k].tobytes() == off[k].tobytes(), (name, k, on[k], off[k])
    # launches of one Solve, (products, vector updates): with the pairs on, one more vector update where the number of
    # iterations is odd -- the update that was outstanding -- and the same number of product launches; with RAMD_CG_XPAIR=0
    # the launches of the loop as it was, one direction update per iteration fewer than the three-launch loop's
    for init in inits:
        tag, it = "_%d" % init[3], int(on["it_%d" % init[3]][0])
        a, b, c = (outs[v]["launches" + tag] for v in ("on", "xpair0", "latdir0"))
        print(tag, it, a, b, c)
        assert a[0] == b[0] == c[0] and a[1] == b[1] + it % 2 and c[1] == b[1] + it, (tag, it, a, b, c)
    return on


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_solves_identical_with_the_switches(tmp_path, shape):
    """CG + Jacobi, 1, 2, 7 and 40 iterations (the odd counts end with the launch that applies the outstanding update): x
    byte-equal, iteration count and residual history equal"""
    on = _solves(tmp_path, shape, [(0.0, 0.0, 1e300, k) for k in (1, 2, 7, 40)])
    for k in (1, 2, 7, 40):
        assert on["it_%d" % k][0] == k and len(on["hist_%d" % k]) >= k, (k, on["it_%d" % k], len(on["hist_%d" % k]))


def test_solve_that_stops_by_tolerance(tmp_path):
    """the stopping rule ends the loop before max_iter, after whichever parity"""
    on = _solves(tmp_path, (192, 17, 4), [(0.0, 1e-6, 1e300, 1000)])
    assert 5 < on["it_1000"][0] < 1000, on["it_1000"]


def test_second_solve_after_an_odd_number_of_iterations(tmp_path):
    """the second Solve of the same solver starts with a deferring launch whatever the first one ended with"""
    on = _solves(tmp_path, (128, 5, 3), [(0.0, 0.0, 1e300, 7)], again=True)
    assert on["it_7"][0] == 7 and on["itt_7"][0] == 7, (on["it_7"], on["itt_7"])
    assert on["xx_7"].tobytes() != on["x_7"].tobytes()


def test_mixed_precision_inner_cg(tmp_path):
    """the fp32 inner CG of MixedPrecisionDC, one Solve per outer iteration on the same built solver: x, outer iterations and
    history equal"""
    outs = []
    for name, env, _ in VARIANTS:
        f = str(tmp_path / ("mp_%s.npz" % name))
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
""" % f, np.float64, env=env)
        outs.append(dict(np.load(f)))
    for other in outs[1:]:
        for k in ("x", "it", "hist"):
            assert outs[0][k].tobytes() == other[k].tobytes(), k


# ================================================================ 5: refusals
def test_refusals():
    """in both modes: every aliasing pair, dtype and size mismatches, a matrix without lattice state 1, a missing form or one
    of kind none, bad slots, a slot_alpha out of range or equal to another slot, a mode that is neither: RAMD_ERR_ARG, nothing
    launched (the vectors and all five slots keep their bytes)"""
    _run(r"""
nx, ny, nz = 128, 5, 3
n = nx * ny * nz
A = mat(*lat(nx, ny, nz, SEVEN)); warm(A, n)
d, _ = dinvs(n)["three"]
h = form(vec(d)); h32 = form(vec(d, np.float32)); hshort = form(vec(d[:n - 64]))
hnone = form(vec(np.random.default_rng(3).uniform(1, 2, n))); assert forminfo(hnone)[0] == 0
x0, p0, r0 = rnd(41, n), rnd(42, n), rnd(43, n)
compare_chains(A, h, x0, p0, rnd(44, n), r0, 2, "the entry works on these operands")
B = mat(*lat(nx, ny, nz, SEVEN))                 # the same operator, never applied: lattice state 0
assert B.LatticeState() == 0 and xready(B, h) == 0
vs = [vec(v) for v in (x0, p0, np.full(n, -5.0), r0, np.full(n, -3.0))]      # x, p_old, p_new, r, q
before = [v.numpy() for v in vs]
ok = (S_RHO, S_PQ, S_NEW, S_ALPHA)
setslots(); s0 = [slotbits(s) for s in range(5)]
call = lambda m, w, f, sl, mode: lib.ramd_fused_cg_direction_apply_dot_xpair(m._h, *[v._h for v in w], f, *sl, mode)
bad = []
for mode in (DEFER, BOTH):
    for i in range(5):                             # every aliasing pair (x too where it is not touched)
        for j in range(i + 1, 5):
            w = list(vs); w[j] = w[i]; bad.append(call(A, w, h, ok, mode))
    for k in range(5):                             # a vector of another type, of another size
        for other in (vec(np.zeros(n), np.float32), vec(np.zeros(n - 64))):
            w = list(vs); w[k] = other; bad.append(call(A, w, h, ok, mode))
    bad += [call(B, vs, h, ok, mode)]              # no lattice state 1
    bad += [call(A, vs, f, ok, mode) for f in (None, hnone, h32, hshort)]
    for k in range(4):                             # a slot out of range, slot_alpha among them
        for v in (-1, 512):
            sl = list(ok); sl[k] = v; bad.append(call(A, vs, h, sl, mode))
    for k in range(3):                             # slot_alpha is one of the other three
        sl = list(ok); sl[3] = sl[k]; bad.append(call(A, vs, h, sl, mode))
    bad += [lib.ramd_fused_cg_direction_apply_dot_xpair(None, *[v._h for v in vs], h, *ok, mode)]
bad += [call(A, vs, h, ok, mode) for mode in (EACH, 3, -1)]
bad += [lib.ramd_fused_cg_direction_apply_dot_xpair_ready(None, h, C.byref(C.c_int())),
        lib.ramd_fused_cg_direction_apply_dot_xpair_ready(A._h, h, None)]
assert len(bad) == 2 * (10 + 10 + 1 + 4 + 8 + 3 + 1) + 3 + 2 and all(s == capi.ERR_ARG for s in bad), bad
for v, w in zip(vs, before):
    same(v.numpy(), w, "refused calls leave the vectors alone")
assert [slotbits(s) for s in range(5)] == s0
assert B.LatticeState() == 0
assert xready(A, None) == 0 and xready(A, hnone) == 0 and xready(A, h32) == 0 and xready(A, hshort) == 0 and xready(A, h) == 1
""")


@pytest.mark.parametrize("env,answers", [({"RAMD_CSR_LAT": "0"}, (0, 0)), ({"RAMD_CG_LATDIR": "0"}, (0, 0)),
                                         ({"RAMD_CG_XPAIR": "0"}, (1, 0))], ids=["CSR_LAT=0", "CG_LATDIR=0", "CG_XPAIR=0"])
def test_queries_with_the_switches(env, answers):
    """the lattice kernel or the fused launch switched off: both queries say no and the entry refuses.  RAMD_CG_XPAIR=0 is
    the solver loop's switch: its query says no, the entry itself still serves a caller that asks for a mode"""
    _run(r"""
nx, ny, nz = 128, 5, 3
n = nx * ny * nz
A = mat(*lat(nx, ny, nz, SEVEN))
h = form(vec(dinvs(n)["uniform"][0]))
p, q = vec(np.ones(n)), vec(np.zeros(n)); capi.check(lib.ramd_fused_apply_dot(A._h, p._h, q._h, S_PQ))
assert (ready(A, h), xready(A, h)) == %r, (ready(A, h), xready(A, h))
if ready(A, h) == 0:
    vs = [vec(v) for v in (rnd(41, n), rnd(42, n), np.full(n, -5.0), rnd(43, n), np.full(n, -3.0))]
    for mode in (DEFER, BOTH):
        assert lib.ramd_fused_cg_direction_apply_dot_xpair(A._h, *[v._h for v in vs], h, S_RHO, S_PQ, S_NEW, S_ALPHA, mode) == capi.ERR_ARG
    same(vs[2].numpy(), np.full(n, -5.0, dtype), "nothing was launched")
else:
    compare_chains(A, h, rnd(41, n), rnd(42, n), rnd(44, n), rnd(43, n), 2, "the entry with the loop's switch off")
""" % (answers,), env=env)
