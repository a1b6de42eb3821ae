"""The fused CG / GMRES / BiCGStab vector kernels of csrc/fused.hip called directly through the C ABI and compared with numpy.

Every headline solve runs through k_cg_update / k_cg_direction (CG) and k_mgs_step / k_mgs_block / k_normalize (the Arnoldi
step of GMRES); the solver tests see them only through whole solves with a history tolerance.  Here:

  A  (test_parity_*)      element by element at the sizes where the 16-byte packet code can go wrong.  The reference is numpy
                          in the vectors' own type, one rounding per operation (the library is built with -ffp-contract=off for
                          exactly this), so vectors are compared BIT FOR BIT.  Reductions: the kernel adds the same fp64 products
                          (double)a * (double)b as numpy forms from the converted elements, only the order differs, and any order
                          of n terms t_i stays within (n - 1) 2^-53 sum|t_i| of the exact sum -- the bound asserted, against the
                          exact sum (math.fsum); nothing is taken from the kernels' own output.
  B  (test_beyond_cap_*)  beyond the cap of the reduction grids (kReduceBlocks = 8192 workgroups of 256 x 4 packets: the
                          grid-stride loop takes a second turn only above 2^24 fp64 / 2^25 fp32 elements) with small dyadic data:
                          every element, every product and every partial sum is exact in any order, so the slots must EQUAL
                          numpy's sums -- a packet left out, taken twice or added to the wrong slot changes the number.
  C                       part A once more in a fresh process with RAMD_NT_STORES=0 and RAMD_MGS_NT=1 (read once per process):
                          the template variants that otherwise run only beyond 256 MB or never; being bit-exact against numpy,
                          part A passing there proves both switches change no bit.
  D                       edges of the entry points: result slots are defined for empty vectors, a written vector may not be
                          passed as another operand, and other bad arguments are refused without touching anything.
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DTYPES = [np.float64, np.float32]
# 1..255: below and around one packet; 1023: the scalar tail of both types; 2047..4097: around one workgroup's share (2048 fp64
# / 4096 fp32 elements); 3*4096+5: the last workgroup has some of its four packets per thread inside and some outside
SIZES = [1, 2, 3, 5, 255, 1023, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 5, 100003]
K_MAX_MULTI_DOT = 8  # kMaxMultiDot of csrc/fused.hip: vectors per launch of multi_dot
MULTI_DOT_COUNTS = [1, 8, 9, 16, 17]  # on each side of every multiple of it up to 17
assert all(m in MULTI_DOT_COUNTS and m + 1 in MULTI_DOT_COUNTS for m in range(K_MAX_MULTI_DOT, 17, K_MAX_MULTI_DOT))
RHO, PQ, NEW, H = 0.731, -1.917, 0.377, 0.613  # (no dyadic values: every coefficient is rounded in the vectors' type)
TR, TT = 0.377, 2.113
SENTINEL = -7.0
# slots of the record as the drivers lay them out (include/rocalution/solvers.hpp)
S_PQ, S_RHO, S_RR, S_NEW = 0, 1, 2, 3  # CG
S_H, S_DOT, S_SQ, S_NRM = 10, 11, 12, 13  # GMRES
S_TR, S_R0Q, S_BRHO, S_BRR, S_BNEW, S_FLAG = 20, 22, 23, 24, 25, 26  # BiCGStab (<t,t> sits at S_TR + 1)


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


def eq(a, b):
    """bit for bit (the sign of a zero included)"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if not np.array_equal(bits(a), bits(b)):
        bad = np.flatnonzero(bits(a) != bits(b))
        raise AssertionError("%d of %d elements differ, first at %d: %r != %r" % (len(bad), a.size, bad[0], a[bad[0]], b[bad[0]]))


def same(x, y):
    """two doubles, bit for bit"""
    return np.float64(x).tobytes() == np.float64(y).tobytes()


def sum_ok(got, a, b, what=""):
    """got against the EXACT sum of the fp64 products t_i = (double)a_i * (double)b_i, within (n - 1) 2^-53 sum|t_i|: what
    any summation order of these products can be off by.  The difference is formed exactly (fsum over the terms and -got)."""
    t = (a.astype(np.float64) * b.astype(np.float64)).tolist()
    bound = (len(t) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in t)
    err = abs(math.fsum(t + [-float(got)]))
    print("%s n=%d got=%.17g err=%.3g bound=%.3g" % (what, len(t), got, err, bound))
    assert err <= bound, (what, got, err, bound)


def mk(rng, n, dtype):
    return rng.uniform(-2.0, 2.0, n).astype(dtype)


# ================================================================ A: parity at the small sizes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_cg_update(ra, dtype, n):
    """alpha = T(rho)/T(pq) ; r' = r + (-alpha) q ; z = dinv r' ; s[rr] = sum r'^2 ; s[rz] = sum r' z, or s[rr] itself
    without a preconditioner (z is then not touched); q and dinv come back unchanged, rho and p.q stay in their slots"""
    lib, capi = _lib()
    rng = np.random.default_rng(1000 + n)
    r0, q0, d0, z0 = (mk(rng, n, dtype) for _ in range(4))
    alpha = dtype(RHO) / dtype(PQ)
    rn = r0 + (-alpha) * q0
    zn = d0 * rn
    assert rn.dtype == dtype and zn.dtype == dtype
    for precond in (True, False):
        r, q, d, z = (ra.LocalVector(dtype, data=v) for v in (r0, q0, d0, z0))
        setslots([(S_RHO, RHO), (S_PQ, PQ), (S_RR, SENTINEL), (S_NEW, SENTINEL)])
        capi.check(lib.ramd_fused_cg_update(r._h, q._h, d._h if precond else None, z._h if precond else None,
                                            S_RHO, S_PQ, S_RR, S_NEW))
        eq(r.numpy(), rn); eq(q.numpy(), q0); eq(d.numpy(), d0)
        s = fetch(0, 4)
        assert s[S_RHO] == RHO and s[S_PQ] == PQ
        sum_ok(s[S_RR], rn, rn, "cg_update rr")
        if precond:
            eq(z.numpy(), zn)
            sum_ok(s[S_NEW], rn, zn, "cg_update rz")
        else:
            eq(z.numpy(), z0)
            assert same(s[S_NEW], s[S_RR]), (s[S_NEW], s[S_RR])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_cg_direction(ra, dtype, n):
    """alpha = T(rho)/T(pq) ; beta = T(new)/T(rho) ; x' = x + alpha p (the OLD p) ; p' = beta p + z ; z comes back unchanged
    and none of the three slots is written"""
    lib, capi = _lib()
    rng = np.random.default_rng(2000 + n)
    x0, p0, z0 = (mk(rng, n, dtype) for _ in range(3))
    x, p, z = (ra.LocalVector(dtype, data=v) for v in (x0, p0, z0))
    setslots([(S_RHO, RHO), (S_PQ, PQ), (S_NEW, NEW), (S_RR, SENTINEL)])
    capi.check(lib.ramd_fused_cg_direction(x._h, p._h, z._h, S_RHO, S_PQ, S_NEW))
    alpha, beta = dtype(RHO) / dtype(PQ), dtype(NEW) / dtype(RHO)
    eq(x.numpy(), x0 + alpha * p0)
    eq(p.numpy(), beta * p0 + z0)
    eq(z.numpy(), z0)
    s = fetch(0, 4)
    assert (s[S_PQ], s[S_RHO], s[S_RR], s[S_NEW]) == (PQ, RHO, SENTINEL, NEW)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_mgs_step(ra, dtype, n):
    """w' = w + (-T(h)) v ; s[dot] = sum u w', or sum w'^2 when u is NULL; v and u come back unchanged.  u == v is legal (both
    are only read) and gives what a copy of v gives."""
    lib, capi = _lib()
    rng = np.random.default_rng(3000 + n)
    w0, v0, u0 = (mk(rng, n, dtype) for _ in range(3))
    wn = w0 + (-dtype(H)) * v0
    assert wn.dtype == dtype
    v, u, vcopy = (ra.LocalVector(dtype, data=a) for a in (v0, u0, v0))
    got = {}
    for form, uvec, uref in (("u", u, u0), ("null", None, wn), ("copy of v", vcopy, v0), ("u == v", v, v0)):
        w = ra.LocalVector(dtype, data=w0)
        setslots([(S_H, H), (S_DOT, SENTINEL)])
        capi.check(lib.ramd_fused_mgs_step(w._h, v._h, S_H, uvec._h if uvec is not None else None, S_DOT))
        eq(w.numpy(), wn)
        s = fetch(S_H, 2)
        assert s[0] == H
        sum_ok(s[1], uref, wn, "mgs_step " + form)
        got[form] = s[1]
    assert same(got["u == v"], got["copy of v"]), got
    eq(v.numpy(), v0); eq(u.numpy(), u0); eq(vcopy.numpy(), v0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_normalize(ra, dtype, n):
    """nrm = T(sqrt(s[sq])) ; inv = T(1)/nrm ; v' = v inv ; s[norm] = nrm, s[sq] is left alone"""
    lib, capi = _lib()
    rng = np.random.default_rng(4000 + n)
    v0 = mk(rng, n, dtype)
    sq = 0.731 + n  # (another square root for every size)
    v = ra.LocalVector(dtype, data=v0)
    setslots([(S_SQ, sq), (S_NRM, SENTINEL)])
    capi.check(lib.ramd_fused_normalize(v._h, S_SQ, S_NRM))
    nrm = dtype(np.sqrt(np.float64(sq)))
    inv = dtype(1) / nrm
    eq(v.numpy(), v0 * inv)
    s = fetch(S_SQ, 2)
    assert s[0] == sq and s[1] == float(nrm), (s, float(nrm))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_bicg_updates(ra, dtype, n):
    """the two BiCGStab updates without a reduction: r' = r + (-alpha) q with alpha = T(rho)/T(r0q), and
    p' = beta p + (-beta omega) q + 1 r with omega = T(tr)/T(tt), beta = (T(new)/T(rho)) (alpha/omega)"""
    lib, capi = _lib()
    rng = np.random.default_rng(5000 + n)
    r0, q0, p0 = (mk(rng, n, dtype) for _ in range(3))
    setslots([(S_BRHO, RHO), (S_R0Q, PQ), (S_TR, TR), (S_TR + 1, TT), (S_BNEW, NEW)])
    alpha, omega = dtype(RHO) / dtype(PQ), dtype(TR) / dtype(TT)
    beta = (dtype(NEW) / dtype(RHO)) * (alpha / omega)
    r, q = ra.LocalVector(dtype, data=r0), ra.LocalVector(dtype, data=q0)
    capi.check(lib.ramd_fused_bicg_r_update(r._h, q._h, S_BRHO, S_R0Q))
    eq(r.numpy(), r0 + (-alpha) * q0); eq(q.numpy(), q0)
    p, r = ra.LocalVector(dtype, data=p0), ra.LocalVector(dtype, data=r0)
    capi.check(lib.ramd_fused_bicg_direction(p._h, q._h, r._h, S_BRHO, S_R0Q, S_TR, S_BNEW))
    eq(p.numpy(), beta * p0 + ((-beta) * omega) * q0 + dtype(1) * r0)
    eq(q.numpy(), q0); eq(r.numpy(), r0)
    s = fetch(S_TR, 6)
    assert tuple(s[[0, 1, 2, 3, 5]]) == (TR, TT, PQ, RHO, NEW)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_parity_multi_dot(ra, dtype, n):
    """s[slot0 + k] = sum v_k w for count vectors, eight per launch: counts on each side of every multiple of eight.  The
    slot behind the last one is not written."""
    lib, capi = _lib()
    rng = np.random.default_rng(6000 + n)
    m = max(MULTI_DOT_COUNTS)
    hv = [mk(rng, n, dtype) for _ in range(m)]
    hw = mk(rng, n, dtype)
    vs = [ra.LocalVector(dtype, data=a) for a in hv]
    w = ra.LocalVector(dtype, data=hw)
    hs = (capi.vec_t * m)(*[v._h for v in vs])
    slot0 = 40
    for count in MULTI_DOT_COUNTS:
        setslots([(slot0 + j, SENTINEL) for j in range(count + 1)])
        capi.check(lib.ramd_fused_multi_dot(hs, count, w._h, slot0))
        s = fetch(slot0, count + 1)
        for j in range(count):
            sum_ok(s[j], hv[j], hw, "multi_dot %d/%d" % (j, count))
        assert s[count] == SENTINEL
    eq(w.numpy(), hw)
    for v, a in zip(vs, hv):
        eq(v.numpy(), a)


PARITY_TESTS = [k for k in list(globals()) if k.startswith("test_parity_")]


# ================================================================ C: the variants behind switches
def test_switched_variants_in_a_fresh_process():
    """RAMD_NT_STORES=0 (k_cg_update<T, true, false>, k_cg_direction<double, false>) and RAMD_MGS_NT=1 (k_mgs_step<..., NTW>,
    the streaming k_mgs_block) are read once per process: part A of this file runs again in ONE fresh interpreter with both
    set.  INTEGRATION.md documents both as changing nothing but speed; part A is bit-exact against numpy."""
    if "RAMD_NT_STORES" in os.environ or "RAMD_MGS_NT" in os.environ:
        pytest.skip("the switches are already set in this process: the selection is running as part A itself")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_parity_"], env=dict(os.environ, RAMD_NT_STORES="0", RAMD_MGS_NT="1"), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    want = len(PARITY_TESTS) * len(SIZES) * len(DTYPES)
    m = re.search(r"(\d+) passed", out)
    assert r.returncode == 0 and m and int(m.group(1)) == want and "skipped" not in out and "failed" not in out, out[-3000:]


# ================================================================ B: beyond the grid cap, exact sums
def exact_dot(a, b):
    """the sum of products of small dyadic numbers: exact in fp64 in any order"""
    return float(np.dot(a.astype(np.float64), b.astype(np.float64)))


@pytest.fixture(scope="module", params=DTYPES, ids=["float64", "float32"])
def big(request, ra):
    """five integer-valued vectors in [-3, 3] and a vector of powers of two in [1/4, 2], on the host (read-only) and on the
    device, one element past two workgroups' second turn with a scalar tail; generated and uploaded once per type"""
    dtype = request.param
    n = (1 << 24) + 2 * 2048 + 3 if dtype is np.float64 else (1 << 25) + 2 * 4096 + 7
    per_turn = 8192 * 256 * 4 * (2 if dtype is np.float64 else 4)
    assert per_turn < n < 2 * per_turn
    rng = np.random.default_rng(7)
    host = [rng.integers(-3, 4, n, dtype=np.int8).astype(dtype) for _ in range(5)]
    host.append(np.ldexp(dtype(1), rng.integers(-2, 2, n, dtype=np.int8)).astype(dtype))
    for a in host:
        a.setflags(write=False)
    dev = [ra.LocalVector(dtype, data=a) for a in host]
    b = types.SimpleNamespace(dtype=dtype, n=n, host=host, dev=dev, V=lambda a: ra.LocalVector(dtype, data=a))
    yield b
    del b.dev[:], b.host[:]


def test_beyond_cap_cg(big):
    """cg_update in both forms and cheb_residual (slots exact), cg_direction (vectors).  rho = 2, p.q = 1, new = 1:
    alpha = 2, beta = 1/2."""
    lib, capi = _lib()
    A, B, Cc, D, E, DINV = big.host
    dA, dB, dC, dD, dE, dDINV = big.dev
    T = big.dtype
    r, z = big.V(A), big.V(np.zeros(big.n, T))
    # preconditioned: r1 = A - 2 B ; z1 = dinv r1
    setslots([(S_RHO, 2.0), (S_PQ, 1.0), (S_RR, SENTINEL), (S_NEW, SENTINEL)])
    capi.check(lib.ramd_fused_cg_update(r._h, dB._h, dDINV._h, z._h, S_RHO, S_PQ, S_RR, S_NEW))
    r1 = A + T(-2) * B
    z1 = DINV * r1
    eq(r.numpy(), r1); eq(z.numpy(), z1)
    s = fetch(0, 4)
    assert s[S_RR] == exact_dot(r1, r1) and s[S_NEW] == exact_dot(r1, z1), s
    # plain: r2 = r1 - 2 B
    setslots([(S_RR, SENTINEL), (S_NEW, SENTINEL)])
    capi.check(lib.ramd_fused_cg_update(r._h, dB._h, None, None, S_RHO, S_PQ, S_RR, S_NEW))
    r2 = r1 + T(-2) * B
    eq(r.numpy(), r2); eq(z.numpy(), z1)
    s = fetch(0, 4)
    assert s[S_RR] == exact_dot(r2, r2) and s[S_NEW] == s[S_RR], s
    del r1
    # direction: x' = C + 2 D ; p' = D / 2 + z1
    x, p = big.V(Cc), big.V(D)
    setslots([(S_NEW, 1.0)])
    capi.check(lib.ramd_fused_cg_direction(x._h, p._h, z._h, S_RHO, S_PQ, S_NEW))
    eq(x.numpy(), Cc + T(2) * D); eq(p.numpy(), T(0.5) * D + z1); eq(z.numpy(), z1)
    del x, p, z, z1
    # residual: r3 = -r2 + E
    setslots([(S_RR, SENTINEL)])
    capi.check(lib.ramd_fused_cheb_residual(r._h, dE._h, S_RR))
    r3 = T(-1) * r2 + E
    eq(r.numpy(), r3)
    assert fetch(S_RR, 1)[0] == exact_dot(r3, r3)


def test_beyond_cap_mgs_step(big):
    """mgs_step with and without u and multi_dot with two vectors (slots exact); normalize and multi_axpy (vectors).  h = 2."""
    lib, capi = _lib()
    A, B, Cc, D, E, _ = big.host
    dA, dB, dC, dD, dE, _ = big.dev
    T = big.dtype
    w = big.V(A)
    setslots([(S_H, 2.0), (S_DOT, SENTINEL)])
    capi.check(lib.ramd_fused_mgs_step(w._h, dB._h, S_H, dC._h, S_DOT))
    w1 = A + T(-2) * B
    eq(w.numpy(), w1)
    assert fetch(S_DOT, 1)[0] == exact_dot(Cc, w1)
    setslots([(S_DOT, SENTINEL)])
    capi.check(lib.ramd_fused_mgs_step(w._h, dC._h, S_H, None, S_DOT))
    w2 = w1 + T(-2) * Cc
    del w1
    eq(w.numpy(), w2)
    assert fetch(S_DOT, 1)[0] == exact_dot(w2, w2)
    hs = (capi.vec_t * 2)(dD._h, dE._h)
    setslots([(40, SENTINEL), (41, SENTINEL), (42, SENTINEL)])
    capi.check(lib.ramd_fused_multi_dot(hs, 2, w._h, 40))
    s = fetch(40, 3)
    assert (s[0], s[1], s[2]) == (exact_dot(D, w2), exact_dot(E, w2), SENTINEL), s
    # normalize: sqrt(16) = 4, w3 = w2 / 4
    setslots([(S_SQ, 16.0), (S_NRM, SENTINEL)])
    capi.check(lib.ramd_fused_normalize(w._h, S_SQ, S_NRM))
    w3 = w2 * (T(1) / T(4))
    del w2
    eq(w.numpy(), w3)
    assert tuple(fetch(S_SQ, 2)) == (16.0, 4.0)
    # multi_axpy: w4 = ((w3 + 2 B) - D / 2) + E
    hs = (capi.vec_t * 3)(dB._h, dD._h, dE._h)
    coef = (C.c_double * 3)(2.0, -0.5, 1.0)
    capi.check(lib.ramd_fused_multi_axpy(w._h, hs, coef, 3))
    eq(w.numpy(), ((w3 + T(2) * B) + T(-0.5) * D) + T(1) * E)


def _mgs_area(npv):
    """sums of a block of npv vectors as a pass leaves them (e_0..e_{npv-1}, then the strict upper triangle of the Gram matrix
    row by row), chosen so that the h of the forward substitution  h_m = e_m - sum_{k<m} h_k g_km  are small dyadic numbers"""
    e = [(1.0, -0.5, 2.0, 0.25)[m % 4] for m in range(npv)]
    g = {(k, m): float((k + m) % 3 - 1) for k in range(npv) for m in range(k + 1, npv)}
    h = list(e)
    for k in range(npv):
        for m in range(k + 1, npv):
            h[m] -= h[k] * g[k, m]
    assert all(abs(v) <= 64 and v * 4 == int(v * 4) for v in h), h
    return e + [g[k, m] for k in range(npv) for m in range(k + 1, npv)], h


def test_beyond_cap_mgs_block(big):
    """mgs_block: a first block (w only read), a middle pass (the previous block applied while the next is projected on) and
    the closing ncur == 0 pass.  The sums a pass leaves are compared exactly; what the NEXT pass reads in their place is set
    from the host so that its h stay small dyadic numbers and every element and sum stays exact."""
    lib, capi = _lib()
    T = big.dtype
    A = big.host[0]
    K = lib.ramd_fused_mgs_block_max()
    # blocks longer than the four basis vectors at hand repeat them (operands that are only read may alias)
    prev_i = [1 + q % 4 for q in range(K)]
    cur1_i = [1 + c % 4 for c in range(K)]
    cur2_i = [4 - c % 4 for c in range(K)]
    handles = lambda idx: (capi.vec_t * len(idx))(*[big.dev[i]._h for i in idx])
    gram = {}

    def vv(i, j):
        if (min(i, j), max(i, j)) not in gram:
            gram[min(i, j), max(i, j)] = exact_dot(big.host[i], big.host[j])
        return gram[min(i, j), max(i, j)]

    def sums(idx, wh):
        return ([exact_dot(big.host[i], wh) for i in idx]
                + [vv(idx[c], idx[d]) for c in range(len(idx)) for d in range(c + 1, len(idx))])

    nsum = K + K * (K - 1) // 2
    area0, area1, slot_h, slot_last = 100, 100 + nsum, 60, 90
    w = big.V(A)
    # first block
    setslots([(area0 + j, SENTINEL) for j in range(nsum)])
    capi.check(lib.ramd_fused_mgs_block(w._h, None, 0, 0, 0, handles(cur1_i), K, area0))
    eq(w.numpy(), A)
    assert fetch(area0, nsum).tolist() == sums(cur1_i, A)
    # middle pass
    flat, h = _mgs_area(K)
    setslots([(area0 + j, v) for j, v in enumerate(flat)] + [(area1 + j, SENTINEL) for j in range(nsum)]
             + [(slot_h + j, SENTINEL) for j in range(K)])
    capi.check(lib.ramd_fused_mgs_block(w._h, handles(prev_i), K, slot_h, area0, handles(cur2_i), K, area1))
    w1 = A
    for q in range(K):
        w1 = w1 + (-T(h[q])) * big.host[prev_i[q]]
    eq(w.numpy(), w1)
    assert fetch(slot_h, K).tolist() == h
    assert fetch(area1, nsum).tolist() == sums(cur2_i, w1)
    # closing pass: a last block of nl vectors applied, s[slot_last] = <w, w>
    nl = max(1, K - 1)
    flat, h = _mgs_area(nl)
    setslots([(area1 + j, v) for j, v in enumerate(flat)] + [(slot_last, SENTINEL)] + [(slot_h + j, SENTINEL) for j in range(nl)])
    capi.check(lib.ramd_fused_mgs_block(w._h, handles(cur2_i[:nl]), nl, slot_h, area1, None, 0, slot_last))
    w2 = w1
    for q in range(nl):
        w2 = w2 + (-T(h[q])) * big.host[cur2_i[q]]
    del w1
    eq(w.numpy(), w2)
    assert fetch(slot_h, nl).tolist() == h
    assert fetch(slot_last, 1)[0] == exact_dot(w2, w2)


def test_beyond_cap_bicgstab(big):
    """bicg_xr_update in both forms (vectors, and the slots exactly), bicg_r_update and bicg_direction (vectors).
    rho = 2, <r0,q> = 1, <t,r> = 1, <t,t> = 2, new = 1: alpha = 2, omega = 1/2, beta = 2."""
    lib, capi = _lib()
    A, B, Cc, D, E, R0 = big.host
    dA, dB, dC, dD, dE, dR0 = big.dev
    T = big.dtype
    x, r = big.V(A), big.V(B)
    base = [(S_BRHO, 2.0), (S_R0Q, 1.0), (S_TR, 1.0), (S_TR + 1, 2.0)]
    clear = [(S_BRR, SENTINEL), (S_BNEW, SENTINEL), (S_FLAG, SENTINEL)]
    # preconditioned: x1 = (1 A + 2 C) + D / 2 ; r1 = B - E / 2     (dir = C, sv = D, t = E, p = C)
    setslots(base + clear)
    capi.check(lib.ramd_fused_bicg_xr_update(x._h, dC._h, dD._h, r._h, dE._h, dR0._h, dC._h, S_BRHO, S_R0Q, S_TR, S_BRR,
                                             S_BNEW, S_FLAG))
    x1 = (T(1) * A + T(2) * Cc) + T(0.5) * D
    r1 = B + T(-0.5) * E
    eq(x.numpy(), x1); eq(r.numpy(), r1)
    s = fetch(S_TR, 7)
    assert (s[4], s[5], s[6]) == (exact_dot(r1, r1), exact_dot(R0, r1), 0.0), s
    assert tuple(s[:4]) == (1.0, 2.0, 1.0, 2.0)
    # plain: dir = p = D, sv = the old r: x2 = (1 x1 + 2 D) + r1 / 2 ; r2 = r1 - E / 2
    setslots(clear)
    capi.check(lib.ramd_fused_bicg_xr_update(x._h, None, None, r._h, dE._h, dR0._h, dD._h, S_BRHO, S_R0Q, S_TR, S_BRR, S_BNEW,
                                             S_FLAG))
    x2 = (T(1) * x1 + T(2) * D) + T(0.5) * r1
    r2 = r1 + T(-0.5) * E
    del x1, r1
    eq(x.numpy(), x2); eq(r.numpy(), r2)
    s = fetch(S_TR, 7)
    assert (s[4], s[5], s[6]) == (exact_dot(r2, r2), exact_dot(R0, r2), 0.0), s
    del x, x2
    # r3 = r2 - 2 D
    capi.check(lib.ramd_fused_bicg_r_update(r._h, dD._h, S_BRHO, S_R0Q))
    r3 = r2 + T(-2) * D
    del r2
    eq(r.numpy(), r3)
    # p' = (2 p - 1 C) + 1 r3      (q = C)
    p = big.V(E)
    setslots([(S_BNEW, 1.0)])
    capi.check(lib.ramd_fused_bicg_direction(p._h, dC._h, r._h, S_BRHO, S_R0Q, S_TR, S_BNEW))
    eq(p.numpy(), (T(2) * E + T(-1) * Cc) + T(1) * r3)
    eq(r.numpy(), r3)


def test_beyond_cap_inputs_untouched(big):
    """the vectors the kernels above only read, after all of them"""
    for d, h in zip(big.dev, big.host):
        eq(d.numpy(), h)


# ================================================================ D: edges of the entry points
def _empty(ra, dtype):
    v = ra.LocalVector(dtype)
    v.Allocate("", 0)
    return v


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_vectors_leave_their_slots_defined(ra, dtype):
    """a rank that owns no rows hands these slots straight to an all-reduce: a sum over no element is 0, never what the slot
    held before"""
    lib, capi = _lib()
    e = [_empty(ra, dtype) for _ in range(7)]
    h = [v._h for v in e]
    for dinv, z in ((h[2], h[3]), (None, None)):
        setslots([(S_RHO, RHO), (S_PQ, PQ), (S_RR, SENTINEL), (S_NEW, SENTINEL)])
        capi.check(lib.ramd_fused_cg_update(h[0], h[1], dinv, z, S_RHO, S_PQ, S_RR, S_NEW))
        assert fetch(0, 4).tolist() == [PQ, RHO, 0.0, 0.0]
    for u in (h[2], None):
        setslots([(S_H, H), (S_DOT, SENTINEL)])
        capi.check(lib.ramd_fused_mgs_step(h[0], h[1], S_H, u, S_DOT))
        assert fetch(S_H, 2).tolist() == [H, 0.0]
    # normalize: the norm is the root of what the slot of the square holds, rounded as for any other size
    setslots([(S_SQ, 0.731), (S_NRM, SENTINEL)])
    capi.check(lib.ramd_fused_normalize(h[0], S_SQ, S_NRM))
    assert fetch(S_SQ, 2).tolist() == [0.731, float(dtype(np.sqrt(np.float64(0.731))))]
    # bicg_xr_update: rr = new = 0, and the flag by the kernel's own rule for every size: omega = T(tr)/T(tt) is formed from
    # the record, the flag is 1 when that omega is 0, NaN or Inf and 0 otherwise
    for tr, tt, flag in ((TR, TT, 0.0), (0.0, TT, 1.0), (TR, 0.0, 1.0), (0.0, 0.0, 1.0)):
        for dir_, sv in ((h[1], h[2]), (None, None)):
            setslots([(S_BRHO, RHO), (S_R0Q, PQ), (S_TR, tr), (S_TR + 1, tt), (S_BRR, SENTINEL), (S_BNEW, SENTINEL),
                      (S_FLAG, SENTINEL)])
            capi.check(lib.ramd_fused_bicg_xr_update(h[0], dir_, sv, h[3], h[4], h[5], h[6], S_BRHO, S_R0Q, S_TR, S_BRR, S_BNEW,
                                                     S_FLAG))
            assert fetch(S_TR, 7).tolist() == [tr, tt, PQ, RHO, 0.0, 0.0, flag], (tr, tt)
    # the entries without a result slot have nothing to do
    capi.check(lib.ramd_fused_cg_direction(h[0], h[1], h[2], S_RHO, S_PQ, S_NEW))
    capi.check(lib.ramd_fused_bicg_r_update(h[0], h[1], S_BRHO, S_R0Q))
    capi.check(lib.ramd_fused_bicg_direction(h[0], h[1], h[2], S_BRHO, S_R0Q, S_TR, S_BNEW))


def _forty(ra, count, dtype=np.float64):
    host = [np.full(40, 1.0 + 0.25 * k, dtype) for k in range(count)]
    return host, [ra.LocalVector(dtype, data=a) for a in host]


def test_written_vectors_may_not_alias_another_operand(ra):
    """the written vectors are __restrict__ pointers next to non-temporal loads of the others: RAMD_ERR_ARG, and nothing is
    touched (slots included); operands that are only read may alias each other"""
    lib, capi = _lib()
    host, vec = _forty(ra, 7)
    a, b, c, d, e, f, g = (v._h for v in vec)
    slots = [(s, 0.5 + s) for s in range(30)]
    setslots(slots)
    bad = []
    cg_update = lambda r, q, dinv, z: lib.ramd_fused_cg_update(r, q, dinv, z, S_RHO, S_PQ, S_RR, S_NEW)
    bad += [cg_update(a, a, c, d), cg_update(a, b, a, d), cg_update(a, b, c, a), cg_update(a, b, c, b), cg_update(a, b, c, c),
            cg_update(a, a, None, None)]
    cg_direction = lambda x, p, z: lib.ramd_fused_cg_direction(x, p, z, S_RHO, S_PQ, S_NEW)
    bad += [cg_direction(a, a, c), cg_direction(a, b, a), cg_direction(a, b, b)]
    mgs_step = lambda w, v, u: lib.ramd_fused_mgs_step(w, v, S_H, u, S_DOT)
    bad += [mgs_step(a, a, c), mgs_step(a, b, a), mgs_step(a, a, None)]
    xr = lambda *v: lib.ramd_fused_bicg_xr_update(*v, S_BRHO, S_R0Q, S_TR, S_BRR, S_BNEW, S_FLAG)
    good = [a, b, c, d, e, f, g]  # x, dir, sv, r, t, r0, p
    for written in (0, 3):
        for other in range(7):
            if other != written:
                args = list(good)
                args[other] = good[written]
                bad.append(xr(*args))
    bad += [xr(a, None, None, d, e, f, a), xr(a, None, None, d, e, d, g), xr(a, None, None, a, e, f, g)]
    bicg_direction = lambda p, q, r: lib.ramd_fused_bicg_direction(p, q, r, S_BRHO, S_R0Q, S_TR, S_BNEW)
    bad += [bicg_direction(a, a, c), bicg_direction(a, b, a)]
    bad += [lib.ramd_fused_bicg_r_update(a, a, S_BRHO, S_R0Q)]
    assert bad == [capi.ERR_ARG] * len(bad), bad
    for v, h0 in zip(vec, host):
        eq(v.numpy(), h0)
    assert fetch(0, 30).tolist() == [v for _, v in slots]
    # read-only operands that alias: q == dinv ; dir == p and sv == t == r0 ; q == r
    capi.check(cg_update(a, b, b, d))
    capi.check(xr(a, b, c, d, c, c, b))
    capi.check(bicg_direction(a, b, b))


def test_bad_arguments_are_refused(ra):
    """mismatched sizes and types, NULL handles and slots outside the record (512 doubles): RAMD_ERR_ARG, nothing touched"""
    lib, capi = _lib()
    host, vec = _forty(ra, 4)
    a, b, c, d = (v._h for v in vec)
    short = ra.LocalVector(data=np.ones(39))
    single = ra.LocalVector(np.float32, data=np.ones(40, np.float32))
    wrong = (short._h, single._h, None)
    slots = [(s, 0.5 + s) for s in range(16)]
    setslots(slots)
    bad = []
    ok4 = (S_RHO, S_PQ, S_RR, S_NEW)
    for x in wrong:
        bad += [lib.ramd_fused_cg_update(x, b, c, d, *ok4), lib.ramd_fused_cg_update(a, x, c, d, *ok4),
                lib.ramd_fused_cg_update(a, b, c, x, *ok4), lib.ramd_fused_cg_update(a, x, None, None, *ok4),
                lib.ramd_fused_cg_update(x, b, None, None, *ok4)]
        if x is not None:  # (dinv == NULL is the form without a preconditioner)
            bad.append(lib.ramd_fused_cg_update(a, b, x, d, *ok4))
        bad += [lib.ramd_fused_cg_direction(x, b, c, S_RHO, S_PQ, S_NEW), lib.ramd_fused_cg_direction(a, x, c, S_RHO, S_PQ, S_NEW),
                lib.ramd_fused_cg_direction(a, b, x, S_RHO, S_PQ, S_NEW)]
        bad += [lib.ramd_fused_mgs_step(x, b, S_H, c, S_DOT), lib.ramd_fused_mgs_step(a, x, S_H, c, S_DOT),
                lib.ramd_fused_mgs_step(x, b, S_H, None, S_DOT)]
        if x is not None:  # (u == NULL: <w, w>)
            bad.append(lib.ramd_fused_mgs_step(a, b, S_H, x, S_DOT))
    bad.append(lib.ramd_fused_normalize(None, S_SQ, S_NRM))
    for s in (-1, 512):
        for k in range(4):
            sl = list(ok4)
            sl[k] = s
            bad += [lib.ramd_fused_cg_update(a, b, c, d, *sl), lib.ramd_fused_cg_update(a, b, None, None, *sl)]
        for k in range(3):
            sl = [S_RHO, S_PQ, S_NEW]
            sl[k] = s
            bad.append(lib.ramd_fused_cg_direction(a, b, c, *sl))
        bad += [lib.ramd_fused_mgs_step(a, b, s, c, S_DOT), lib.ramd_fused_mgs_step(a, b, S_H, c, s),
                lib.ramd_fused_mgs_step(a, b, s, None, S_DOT), lib.ramd_fused_mgs_step(a, b, S_H, None, s)]
        bad += [lib.ramd_fused_normalize(a, s, S_NRM), lib.ramd_fused_normalize(a, S_SQ, s)]
    bad.append(lib.ramd_fused_normalize(a, S_SQ, S_SQ))  # (the norm would overwrite the square other workgroups still read)
    assert bad == [capi.ERR_ARG] * len(bad), bad
    for v, h0 in zip(vec, host):
        eq(v.numpy(), h0)
    eq(short.numpy(), np.ones(39)); eq(single.numpy(), np.ones(40, np.float32))
    assert fetch(0, 16).tolist() == [v for _, v in slots]
