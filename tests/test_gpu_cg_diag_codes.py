"""CG + Jacobi with the inverse diagonal in its coded form and z never stored (csrc/fused.hip: ramd_dcode_*,
ramd_fused_cg_update_dc, ramd_fused_cg_direction_dc), through the C ABI.

Every expected value comes from the EXISTING entry points ramd_fused_cg_update / ramd_fused_cg_direction run on the same
inputs -- never from the kernels under test -- and is compared without a tolerance: vectors as bytes, slots as bits.

  1  kernel parity at the sizes of the packet, tail and stream-loop edges, both types, three kinds of inverse diagonal
  2  beyond the cap of the reduction grid (a second turn of the grid-stride loop), both kinds, small dyadic data
  3  the build of the coded form: kinds, the 256 / 257 boundary, signed zeros, NaN payloads, inf, order of the table, codes
  4  bad arguments are refused with RAMD_ERR_ARG
  5  whole solves in fresh processes with RAMD_CG_DCODE=0 and =1 (the switch is read once): identical x, iteration count
     and residual history, fp64 and fp32, for a uniform, a coded and an uncodable diagonal
  6  the same for a Global run, two ranks on one device over the callback transport
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_dcode_worker.py")

DTYPES = [np.float64, np.float32]
# the sizes tests/test_gpu_fused_vector_kernels.py found sufficient: below and around one packet, the scalar tail of both
# types, around one workgroup's share (2048 fp64 / 4096 fp32 elements), a last workgroup with some of its packets outside
SIZES = [1, 2, 3, 5, 255, 1023, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5, 100003]
RHO, PQ = 0.731, -1.917  # (no dyadic values: every coefficient is rounded in the vectors' type)
SENTINEL = -7.0
S_PQ, S_RHO, S_RR, S_NEW = 0, 1, 2, 3  # slots as CG lays them out (include/rocalution/solvers.hpp)
NONE, UNIFORM, CODED = 0, 1, 2  # RAMD_DCODE_*


@pytest.fixture(scope="module")
def ra():
    import rocalution_amd as ra
    ra.init_rocalution()
    return ra


def _lib():
    from rocalution_amd import capi
    return capi.load(), capi


def setslots(pairs):
    lib, capi = _lib()
    for s, v in pairs:
        capi.check(lib.ramd_scalars_set(s, float(v)))


def fetch(first, count):
    lib, capi = _lib()
    out = np.zeros(count)
    capi.check(lib.ramd_scalars_fetch(out.ctypes.data_as(capi.pf64), first, count))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(bits(a) != bits(b))
        raise AssertionError("%s: %d of %d elements differ, first at %d: %r != %r" % (what, len(bad), a.size, bad[0], a[bad[0]], b[bad[0]]))


class Form:
    """a coded form built from a device vector; destroyed with the object"""

    def __init__(self, vec):
        lib, capi = _lib()
        self.h = C.c_void_p()
        self.status = lib.ramd_dcode_create_from_vector(vec._h if vec is not None else None, C.byref(self.h))
        self.dtype = vec.dtype if vec is not None else None

    def info(self):
        lib, capi = _lib()
        kind, count, n = C.c_int(-1), C.c_int(-1), C.c_int64(-1)
        capi.check(lib.ramd_dcode_info(self.h, C.byref(kind), C.byref(count), C.byref(n)))
        return kind.value, count.value, n.value

    def host(self):
        """(table, codes) copied back; codes is None unless the kind is coded"""
        lib, capi = _lib()
        kind, count, n = self.info()
        table = np.zeros(count, self.dtype)
        codes = np.full(n, 255, np.uint8) if kind == CODED else None
        capi.check(lib.ramd_dcode_copy_to_host(self.h, table.ctypes.data_as(C.c_void_p),
                                               codes.ctypes.data_as(C.c_void_p) if codes is not None else None))
        return table, codes

    def __del__(self):
        try:
            if self.h:
                _lib()[0].ramd_dcode_destroy(self.h)
                self.h = None
        except Exception:
            pass


def run_old(ra, dtype, r0, q0, d0, x0, p0, new=None):
    """the existing pair on fresh copies -> r, x, p, (rr, rz); s[new] is what the residual update left unless `new` is given"""
    lib, capi = _lib()
    r, q, d, z, x, p = (ra.LocalVector(dtype, data=v) for v in (r0, q0, d0, np.zeros_like(r0), x0, p0))
    setslots([(S_RHO, RHO if new is None else 2.0), (S_PQ, PQ if new is None else 1.0), (S_RR, SENTINEL), (S_NEW, SENTINEL)])
    capi.check(lib.ramd_fused_cg_update(r._h, q._h, d._h, z._h, S_RHO, S_PQ, S_RR, S_NEW))
    s = fetch(0, 4)
    if new is not None:
        setslots([(S_NEW, new)])
    capi.check(lib.ramd_fused_cg_direction(x._h, p._h, z._h, S_RHO, S_PQ, S_NEW))
    return r.numpy(), x.numpy(), p.numpy(), s[[S_RR, S_NEW]]


def run_new(ra, dtype, r0, q0, form, x0, p0, new=None):
    lib, capi = _lib()
    r, q, x, p = (ra.LocalVector(dtype, data=v) for v in (r0, q0, x0, p0))
    setslots([(S_RHO, RHO if new is None else 2.0), (S_PQ, PQ if new is None else 1.0), (S_RR, SENTINEL), (S_NEW, SENTINEL)])
    capi.check(lib.ramd_fused_cg_update_dc(r._h, q._h, form.h, S_RHO, S_PQ, S_RR, S_NEW))
    s = fetch(0, 4)
    assert s[S_RHO] == (RHO if new is None else 2.0) and s[S_PQ] == (PQ if new is None else 1.0)
    if new is not None:
        setslots([(S_NEW, new)])
    capi.check(lib.ramd_fused_cg_direction_dc(x._h, p._h, r._h, form.h, S_RHO, S_PQ, S_NEW))
    same_bytes(q.numpy(), q0, "q is only read")
    return r.numpy(), x.numpy(), p.numpy(), s[[S_RR, S_NEW]]


def compare(old, new, what):
    for name, a, b in zip(("r", "x", "p"), old[:3], new[:3]):
        same_bytes(a, b, "%s %s" % (what, name))
    print(what, "rr", old[3][0], new[3][0], "rz", old[3][1], new[3][1])
    assert bits(old[3]).tolist() == bits(new[3]).tolist(), (what, old[3], new[3])


def dinv_ways(rng, n, dtype):
    """the three inverse diagonals of part 1: one value; three values placed irregularly; 256 distinct values (as many as
    fit, below 256 elements), every one of them present"""
    three = np.array([1.0 / 6.0, 1.0 / 12.0, 0.37], dtype)
    many = (0.05 + np.arange(256) / 300.0).astype(dtype)
    assert len(np.unique(bits(many))) == 256
    spread = np.concatenate([many[:min(n, 256)], rng.choice(many, max(n - 256, 0))])
    return {"one": np.full(n, dtype(1.0 / 6.0), dtype), "three": rng.choice(three, n), "many": rng.permutation(spread)}


# ================================================================ 1: kernel parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_vector_kernels(ra, dtype, n):
    rng = np.random.default_rng(4000 + n)
    r0, q0, x0, p0 = (rng.uniform(-2.0, 2.0, n).astype(dtype) for _ in range(4))
    for way, d0 in dinv_ways(rng, n, dtype).items():
        distinct = len(np.unique(bits(d0)))
        form = Form(ra.LocalVector(dtype, data=d0))
        assert form.status == 0
        assert form.info() == (UNIFORM if distinct == 1 else CODED, distinct, n), (way, form.info())
        if way == "many" and n >= 256:
            assert distinct == 256
        old = run_old(ra, dtype, r0, q0, d0, x0, p0)
        new = run_new(ra, dtype, r0, q0, form, x0, p0)
        compare(old, new, "%s n=%d %s" % (np.dtype(dtype).name, n, way))


# ================================================================ 2: beyond the cap of the reduction grid
@pytest.fixture(scope="module")
def big():
    """integer-valued vectors in [-3, 3], one element class past the first turn of the capped grid (8192 workgroups of
    256 x 4 packets of 2 fp64 elements = 2^24) with a scalar tail; generated once, read-only"""
    n = (1 << 24) + 4099
    rng = np.random.default_rng(7)
    host = [rng.integers(-3, 4, n, dtype=np.int8).astype(np.float64) for _ in range(4)]
    pow2 = np.ldexp(1.0, rng.integers(-2, 2, n, dtype=np.int8)).astype(np.float64)
    for a in host + [pow2]:
        a.setflags(write=False)
    b = types.SimpleNamespace(n=n, host=host, pow2=pow2)
    yield b
    del b.host[:], b.pow2


@pytest.mark.parametrize("kind", ["uniform", "coded"])
def test_beyond_cap(ra, big, kind):
    """rho = 2, p.q = 1: alpha = 2; s[new] = 1 for the direction update: beta = 1/2 -- every element, product and partial sum
    is exact in any order"""
    d0 = np.full(big.n, 0.5) if kind == "uniform" else big.pow2
    form = Form(ra.LocalVector(np.float64, data=d0))
    assert form.info() == ((UNIFORM, 1, big.n) if kind == "uniform" else (CODED, 4, big.n))
    old = run_old(ra, np.float64, *big.host[:2], d0, *big.host[2:], new=1.0)
    new = run_new(ra, np.float64, *big.host[:2], form, *big.host[2:], new=1.0)
    compare(old, new, "beyond cap %s" % kind)
    r1 = big.host[0] - 2.0 * big.host[1]  # (and the old path is what it has always been)
    assert old[3][0] == float(np.dot(r1, r1)) and old[3][1] == float(np.dot(r1, d0 * r1))


# ================================================================ 3: the build of the coded form
@pytest.mark.parametrize("dtype", DTYPES)
def test_build_of_the_coded_form(ra, dtype):
    U = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    rng = np.random.default_rng(11)

    def form_of(values):
        v = np.ascontiguousarray(values, dtype=dtype)
        f = Form(ra.LocalVector(dtype, data=v))
        assert f.status == 0
        return f, v

    def check_round_trip(f, v, count):
        assert f.info() == (CODED, count, len(v))
        table, codes = f.host()
        tb = bits(table).astype(np.uint64)
        assert np.all(tb[1:] > tb[:-1]), "table sorted ascending by bits, no entry twice"
        assert tb.tolist() == np.unique(bits(v)).astype(np.uint64).tolist()
        assert codes.max() < count
        same_bytes(table[codes], v, "table[code[i]] == v[i]")

    base = (1.0 + np.arange(257) / 512.0).astype(dtype)
    assert len(np.unique(bits(base))) == 257
    # 256 distinct values: coded, count 256; 257: none
    f, v = form_of(rng.permutation(np.concatenate([base[:256], rng.choice(base[:256], 5000)])))
    check_round_trip(f, v, 256)
    f, v = form_of(rng.permutation(np.concatenate([base, rng.choice(base, 5000)])))
    assert f.info() == (NONE, 0, len(v))
    f, v = form_of(rng.uniform(1, 2, 100003))
    assert f.info() == (NONE, 0, len(v))
    # +0.0 and -0.0 are two entries
    f, v = form_of(rng.choice(np.array([0.0, -0.0], dtype), 3001))
    check_round_trip(f, v, 2)
    # two NaNs with different payloads are two entries; inf (the inverse of a zero diagonal) is kept as it is
    quiet = {4: 0x7FC00000, 8: 0x7FF8000000000000}[np.dtype(dtype).itemsize]
    nans = np.array([quiet | 1, quiet | 2], U).view(dtype)
    f, v = form_of(rng.choice(nans, 3001))
    check_round_trip(f, v, 2)
    f, v = form_of(rng.choice(np.concatenate([nans, np.array([np.inf, -np.inf, 0.25, -3.0], dtype)]), 4097))
    check_round_trip(f, v, 6)
    f, v = form_of(np.full(777, np.inf))
    assert f.info() == (UNIFORM, 1, 777)
    assert bits(f.host()[0]).tolist() == bits(np.array([np.inf], dtype)).tolist()
    if dtype is np.float64:  # the one pattern that equals the dictionary's empty mark
        ones = np.array([0xFFFFFFFFFFFFFFFF, 0x3FF0000000000000], np.uint64).view(np.float64)
        f, v = form_of(rng.choice(ones, 3001))
        check_round_trip(f, v, 2)
        f, v = form_of(np.full(300, ones[0]))
        assert f.info() == (UNIFORM, 1, 300) and bits(f.host()[0])[0] == 0xFFFFFFFFFFFFFFFF
    # n = 0: none; n = 1: uniform
    empty = ra.LocalVector(dtype)
    f = Form(empty)
    assert f.status == 0 and f.info() == (NONE, 0, 0)
    f, v = form_of([0.37])
    assert f.info() == (UNIFORM, 1, 1)
    same_bytes(f.host()[0], v, "the uniform value")


# ================================================================ 4: bad arguments
def test_bad_arguments_are_refused(ra):
    lib, capi = _lib()
    n = 1000
    mk = lambda dt, m=n: ra.LocalVector(dt, data=np.full(m, 0.5, dt))
    a, b, c = mk(np.float64), mk(np.float64), mk(np.float64)
    f64, f32, short = Form(mk(np.float64)), Form(mk(np.float32)), Form(mk(np.float64, n - 1))
    none = Form(ra.LocalVector(np.float64, data=np.random.default_rng(3).uniform(1, 2, n)))
    assert none.info()[0] == NONE
    ok4, ok3 = (S_RHO, S_PQ, S_RR, S_NEW), (S_RHO, S_PQ, S_NEW)
    setslots([(S_RHO, RHO), (S_PQ, PQ), (S_NEW, 0.377)])
    before = [v.numpy() for v in (a, b, c)]
    bad = []
    # the form: another size, another type, holding nothing, missing
    for f in (short.h, f32.h, none.h, None):
        bad += [lib.ramd_fused_cg_update_dc(a._h, b._h, f, *ok4), lib.ramd_fused_cg_direction_dc(a._h, b._h, c._h, f, *ok3)]
    # vectors of another size or type
    for other in (mk(np.float64, n - 1), mk(np.float32)):
        bad += [lib.ramd_fused_cg_update_dc(a._h, other._h, f64.h, *ok4), lib.ramd_fused_cg_update_dc(other._h, b._h, f64.h, *ok4),
                lib.ramd_fused_cg_direction_dc(other._h, b._h, c._h, f64.h, *ok3),
                lib.ramd_fused_cg_direction_dc(a._h, other._h, c._h, f64.h, *ok3),
                lib.ramd_fused_cg_direction_dc(a._h, b._h, other._h, f64.h, *ok3)]
    # a written vector passed as another operand
    bad += [lib.ramd_fused_cg_update_dc(a._h, a._h, f64.h, *ok4), lib.ramd_fused_cg_direction_dc(a._h, a._h, c._h, f64.h, *ok3),
            lib.ramd_fused_cg_direction_dc(a._h, b._h, a._h, f64.h, *ok3), lib.ramd_fused_cg_direction_dc(a._h, b._h, b._h, f64.h, *ok3)]
    # slots out of range
    for k in range(4):
        for v in (-1, 512):
            sl = list(ok4); sl[k] = v
            bad.append(lib.ramd_fused_cg_update_dc(a._h, b._h, f64.h, *sl))
    for k in range(3):
        for v in (-1, 512):
            sl = list(ok3); sl[k] = v
            bad.append(lib.ramd_fused_cg_direction_dc(a._h, b._h, c._h, f64.h, *sl))
    # the build: no vector, no place for the handle, not a real vector
    h = C.c_void_p()
    ints = ra.LocalVector(np.int32, data=np.arange(5, dtype=np.int32))
    bad += [lib.ramd_dcode_create_from_vector(None, C.byref(h)), lib.ramd_dcode_create_from_vector(a._h, None),
            lib.ramd_dcode_create_from_vector(ints._h, C.byref(h)), lib.ramd_dcode_info(None, None, None, None)]
    assert bad and all(s == capi.ERR_ARG for s in bad), bad
    for v, w in zip((a, b, c), before):  # nothing was touched
        same_bytes(v.numpy(), w, "refused calls leave the vectors alone")
    assert lib.ramd_dcode_destroy(None) == 0


# ================================================================ 5: whole solves, the switch off and on
def _solve_in_fresh_process(case, switch):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "out.npz")
        subprocess.run([sys.executable, WORKER, "local", case, out], env=dict(os.environ, RAMD_CG_DCODE=switch), check=True,
                       timeout=300)
        return dict(np.load(out))


@pytest.mark.parametrize("case,kind,count", [("a", UNIFORM, 1), ("b", CODED, 3), ("c", NONE, 0)])
def test_solves_identical_with_the_switch_off_and_on(case, kind, count):
    off, on = _solve_in_fresh_process(case, "0"), _solve_in_fresh_process(case, "1")
    for tag in ("64", "32"):
        assert on["form" + tag][:2].tolist() == [kind, count], (case, tag, on["form" + tag])
        print(case, tag, "iterations", on["it" + tag], "history", len(on["hist" + tag]))
        assert on["it" + tag][0] > 5
        for key in ("x", "it", "hist"):
            same_bytes(off[key + tag], on[key + tag], "case %s fp%s %s" % (case, tag, key))
    if case == "a":  # (the golden history of this operator, so that neither run is vacuous)
        gold = np.load(os.path.join(ROOT, "tests", "golden", "poisson16.npz"))["cg_jacobi_meta"]
        print("golden meta", gold)


# ================================================================ 6: a Global run
def _global_run(switch, world=2):
    with tempfile.TemporaryDirectory() as d:
        initfile = os.path.join(d, "init")
        procs = [subprocess.Popen([sys.executable, WORKER, "global", str(r), str(world), initfile, d],
                                  env=dict(os.environ, RAMD_CG_DCODE=switch)) for r in range(world)]
        for p in procs:
            assert p.wait(timeout=300) == 0
        return [dict(np.load(os.path.join(d, "r%d.npz" % r))) for r in range(world)]


def test_global_run_identical_with_the_switch_off_and_on():
    off, on = _global_run("0"), _global_run("1")
    for r, (a, b) in enumerate(zip(off, on)):
        assert b["it"][0] > 5, b["it"]
        for key in ("xs", "it", "res"):
            same_bytes(a[key], b[key], "rank %d %s" % (r, key))
    xs = np.concatenate([b["xs"] for b in on])
    assert np.linalg.norm(xs - 1.0) / np.sqrt(len(xs)) < 1e-6  # (rhs = A 1)
