"""Plain numpy restatement of the BlockPreconditioner (tests only), written after the reference's statements
(preconditioner_blockprecond.cpp): Build (:188-296) -- the offsets, the permuted operator (LocalMatrix::Permute), the blocks
by the ExtractSubMatrix rule of tests/_schwarz_ref.py -- and Solve (:298-391) -- CopyFromPermute / the slice copies, per block
row the ApplyAdd calls with the scalar -1 for j ascending, the block solve, the slice copies back and CopyFromPermuteBackward.
ApplyAdd is host_matrix_csr.cpp:759-767: out[i] += scalar * val * in[col] entry by entry in storage order, every product and
sum rounded in the value type."""
import numpy as np

from _schwarz_ref import extract


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])


def permute(rp, ci, va, perm):
    """LocalMatrix::Permute (host_matrix_csr.cpp): row perm[i] of the result is row i, its columns perm[col], sorted by the
    new column (insertion sort: entries of equal column keep their order)"""
    n = len(rp) - 1
    rows = [None] * n
    for i in range(n):
        cols = np.asarray(perm)[ci[rp[i]:rp[i + 1]]]
        order = np.argsort(cols, kind="stable")
        rows[perm[i]] = (cols[order], np.asarray(va[rp[i]:rp[i + 1]])[order])
    orp = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
    oci = np.concatenate([r[0] for r in rows]).astype(np.int32) if n else np.zeros(0, np.int32)
    ova = np.concatenate([r[1] for r in rows]).astype(va.dtype) if n else np.zeros(0, va.dtype)
    return orp, oci, ova


def build(rp, ci, va, sizes, perm=None):
    """-> blocks[i][j] for j <= i (CSR triples); the upper blocks are cleared by Build() and never used"""
    off = offsets(sizes)
    assert off[-1] == len(rp) - 1 and all(s >= 1 for s in sizes)
    if perm is not None:
        assert len(perm) == len(rp) - 1
        rp, ci, va = permute(rp, ci, va, perm)
    nb = len(sizes)
    return [[extract(rp, ci, va, int(off[i]), int(off[j]), int(sizes[i]), int(sizes[j])) for j in range(i + 1)] for i in range(nb)]


def apply_add(block, x, scalar, y):
    """y += scalar * A x, term by term into y (in place)"""
    rp, ci, va = block
    if len(ci) == 0:
        return
    t = y.dtype.type
    scalar = t(scalar)
    for i in range(len(rp) - 1):
        acc = y[i]
        for k in range(rp[i], rp[i + 1]):
            acc = t(acc + t(t(scalar * va[k]) * x[ci[k]]))
        y[i] = acc


def permuted_rhs(rhs, perm):
    """CopyFromPermute: dst[perm[i]] = src[i]"""
    if perm is None:
        return rhs.copy()
    out = np.empty_like(rhs)
    out[np.asarray(perm)] = rhs
    return out


def step(blocks, sizes, b, rhs, z, perm=None, diag_only=False):
    """the right-hand side of block row b: the slice of the (permuted) rhs, minus the lower blocks times the earlier
    solutions z[0 .. b - 1] unless diag_only"""
    off = offsets(sizes)
    r = permuted_rhs(rhs, perm)[off[b]:off[b + 1]].copy()
    if not diag_only:
        for j in range(b):
            apply_add(blocks[b][j], z[j], -1, r)
    return r


def join(z, perm=None):
    """the slice copies and CopyFromPermuteBackward: dst[i] = src[perm[i]]"""
    x = np.concatenate(z)
    return x.copy() if perm is None else x[np.asarray(perm)]


def solve(blocks, sizes, rhs, local_solve, perm=None, diag_only=False):
    """one apply; local_solve(b, r_b) -> z_b stands for D_solver[b]->SolveZeroSol"""
    z = []
    for b in range(len(sizes)):
        z.append(local_solve(b, step(blocks, sizes, b, rhs, z, perm, diag_only)))
    return join(z, perm)
