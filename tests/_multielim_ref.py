"""Plain numpy restatement of what MultiElimination is made of (tests only): the sequential independent-set sweep
(host_matrix_csr.cpp:2602-2663), Compress (:3679-3740), and one level's Solve
(preconditioner_multielimination.cpp:312-342) given the operator, the permutation and the Schur complement's arrays, with
Jacobi as the last-block solver.  Every product and sum is rounded in the value type, in the reference's order."""
import numpy as np


def sweep(rp, ci):
    """-> (size, perm, members): the first undecided row joins and marks every off-diagonal column of its row as out, also a
    column that had already joined; members first, in order, then the rest.  members < size: the sweep overwrote members
    and perm is no permutation"""
    n = len(rp) - 1
    mis = np.zeros(n, np.int64)
    size = 0
    for i in range(n):
        if mis[i] == 0:
            mis[i] = 1
            size += 1
            for j in range(rp[i], rp[i + 1]):
                if ci[j] != i:
                    mis[ci[j]] = -1
    perm = np.zeros(n, np.int32)
    pos = 0
    for i in range(n):
        if mis[i] == 1:
            perm[i] = pos
            pos += 1
        else:
            perm[i] = size + i - pos
    return size, perm, pos


def fixed_point(rp, ci):
    """the parallel restatement for a structurally symmetric pattern -> (state, rounds): a row is out once a lower-numbered
    neighbour has joined and joins once every lower-numbered neighbour is out (synchronous rounds)"""
    n = len(rp) - 1
    state = np.zeros(n, np.int64)
    rounds = 0
    while (state == 0).any():
        new = state.copy()
        for i in np.nonzero(state == 0)[0]:
            nb = ci[rp[i]:rp[i + 1]]
            nb = nb[nb < i]
            if (state[nb] == 1).any():
                new[i] = -1
            elif (state[nb] == -1).all():
                new[i] = 1
        state = new
        rounds += 1
    return state, rounds


def compress(rp, ci, va, drop):
    """-> (rp, ci, va): an entry stays if |val| > drop (in double) or it is on the diagonal"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    keep = (np.abs(va.astype(np.float64)) > drop) | (ci == rows)
    orp = np.zeros(len(rp), np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=len(rp) - 1), out=orp[1:])
    return orp, ci[keep].astype(np.int32), va[keep]


def permute(rp, ci, va, perm):
    """P A P^T as LocalMatrix::Permute builds it (:3848-3958): row perm[i] is row i, columns renumbered and put in ascending
    order by a stable insertion"""
    n = len(rp) - 1
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    orp, oci, ova = [0], [], []
    for k in range(n):
        i = inv[k]
        c = perm[ci[rp[i]:rp[i + 1]]]
        o = np.argsort(c, kind="stable")
        oci.extend(c[o]); ova.extend(va[rp[i]:rp[i + 1]][o])
        orp.append(len(oci))
    return np.array(orp, np.int32), np.array(oci, np.int32), np.array(ova, va.dtype)


def submatrix(rp, ci, va, r0, c0, rs, cs):
    orp, oci, ova = [0], [], []
    for i in range(r0, r0 + rs):
        for j in range(rp[i], rp[i + 1]):
            if c0 <= ci[j] < c0 + cs:
                oci.append(ci[j] - c0); ova.append(va[j])
        orp.append(len(oci))
    return np.array(orp, np.int32), np.array(oci, np.int32), np.array(ova, va.dtype)


def apply_add(rp, ci, va, x, scalar, y):
    """y[i] += scalar * val * x[col], entry by entry (host_matrix_csr.cpp:737-769)"""
    dt = va.dtype.type
    for i in range(len(rp) - 1):
        for j in range(rp[i], rp[i + 1]):
            y[i] = dt(y[i] + dt(dt(dt(scalar) * va[j]) * x[ci[j]]))
    return y


def diagonal(rp, ci, va):
    d = np.zeros(len(rp) - 1, va.dtype)
    for i in range(len(rp) - 1):
        for j in range(rp[i], rp[i + 1]):
            if ci[j] == i:
                d[i] = va[j]
                break
    return d


def blocks(rp, ci, va, perm, size):
    """-> (inv_D, E D^-1, F) of the permuted operator, each matrix as (rp, ci, va)"""
    n = len(rp) - 1
    dt = va.dtype.type
    P = permute(rp, ci, va, perm)
    D = submatrix(*P, 0, 0, size, size)
    inv_d = (dt(1) / diagonal(*D)).astype(va.dtype)
    F = submatrix(*P, 0, size, size, n - size)
    E = submatrix(*P, size, 0, n - size, size)
    E = (E[0], E[1], (E[2] * inv_d[E[1]]).astype(va.dtype))
    return inv_d, E, F


def solve_level1(rp, ci, va, perm, size, aa, rhs):
    """one elimination with Jacobi on AA = (rp, ci, va): the reference's Solve step by step"""
    n = len(rp) - 1
    dt = va.dtype.type
    inv_d, E, F = blocks(rp, ci, va, perm, size)
    rhs_ = np.empty(n, va.dtype)
    rhs_[perm] = rhs.astype(va.dtype)
    x1, rhs2 = rhs_[:size].copy(), rhs_[size:].copy()
    apply_add(*E, x1, -1, rhs2)
    x2 = (rhs2 * (dt(1) / diagonal(*aa)).astype(va.dtype)).astype(va.dtype)
    apply_add(*F, x2, -1, x1)
    x1 = (x1 * inv_d).astype(va.dtype)
    x_ = np.concatenate([x1, x2])
    return x_[perm]
