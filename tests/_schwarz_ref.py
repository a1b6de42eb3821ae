"""Plain numpy restatement of what AS / RAS are made of (tests only), written after the reference's loops
(preconditioner_as.cpp): the layout (Build :117-131), the weights (:133-156), the restriction (Solve :246-249), the AS join
(:258-269: Zeros, ScaleAddScale(1, z_i, 1) for i ascending, PointWiseMult) and the RAS join (:363-370), every sum and
product rounded in the value type and taken in the reference's order; and the direct sum of the diagonal blocks."""
import numpy as np


def layout(n, nb, ov):
    """-> (size, pos, sizes), or ValueError where the reference's Build() would assert or overrun the matrix"""
    if nb < 1:
        raise ValueError("nb < 1")
    if ov < 0:
        raise ValueError("overlap < 0")
    size = n // nb
    if size < 1:
        raise ValueError("n / nb < 1")
    pos, sizes = [0] * nb, [0] * nb
    offset = 0
    for i in range(nb):
        pos[i] = offset - ov
        offset += size
        sizes[i] = size + 2 * ov
    pos[0] = 0
    sizes[0] = size + ov
    sizes[nb - 1] = size + ov
    if any(p < 0 for p in pos):
        raise ValueError("a block starts before row 0")
    if any(p + s > n for p, s in zip(pos, sizes)):
        raise ValueError("a block overruns the matrix")
    return size, np.array(pos, np.int64), np.array(sizes, np.int64)


def weights(n, nb, ov, dtype):
    size, pos, _ = layout(n, nb, ov)
    w = np.ones(n, dtype)
    for i in range(nb):
        for j in range(ov):
            if i != 0:
                w[pos[i] + j] = 0.5
            if i != nb - 1:
                w[pos[i] + size + j] = 0.5
    return w


def split(rhs, nb, ov):
    """-> the nb pieces r_i = rhs[pos_i : pos_i + sizes_i] (copies)"""
    _, pos, sizes = layout(len(rhs), nb, ov)
    return [rhs[p:p + s].copy() for p, s in zip(pos, sizes)]


def join_as(z, n, nb, ov):
    dtype = z[0].dtype
    _, pos, sizes = layout(n, nb, ov)
    one = dtype.type(1)
    x = np.zeros(n, dtype)
    for i in range(nb):
        seg = slice(pos[i], pos[i] + sizes[i])
        x[seg] = one * x[seg] + one * z[i]
    return x * weights(n, nb, ov, dtype)


def join_ras(z, x, nb, ov):
    """writes into x (the rows of no block keep what they held) and returns it"""
    size, pos, _ = layout(len(x), nb, ov)
    z_offset = 0
    for i in range(nb):
        x[pos[i] + z_offset:pos[i] + z_offset + size] = z[i][z_offset:z_offset + size]
        z_offset = ov
    return x


def extract(rp, ci, va, r0, c0, rs, cs):
    """ExtractSubMatrix (host_matrix_csr.cpp:848-916): order within a row unchanged"""
    orp, oci, ova = [0], [], []
    for i in range(rs):
        for j in range(rp[r0 + i], rp[r0 + i + 1]):
            if c0 <= ci[j] < c0 + cs:
                oci.append(ci[j] - c0)
                ova.append(va[j])
        orp.append(len(oci))
    return np.array(orp, np.int32), np.array(oci, np.int32), np.array(ova, va.dtype)


def blocks(rp, ci, va, nb, ov):
    _, pos, sizes = layout(len(rp) - 1, nb, ov)
    return [extract(rp, ci, va, int(p), int(p), int(s), int(s)) for p, s in zip(pos, sizes)]


def direct_sum(parts):
    """block-diagonal assembly of CSR triples -> (rowptr, col, val)"""
    rp, ci, va, row0, nz0 = [np.zeros(1, np.int32)], [], [], 0, 0
    for brp, bci, bva in parts:
        rp.append(brp[1:] + nz0)
        ci.append(bci + row0)
        va.append(bva)
        row0 += len(brp) - 1
        nz0 += len(bci)
    return np.concatenate(rp).astype(np.int32), np.concatenate(ci).astype(np.int32), np.concatenate(va)


def dense(rp, ci, va):
    n = len(rp) - 1
    A = np.zeros((n, n), va.dtype)
    for i in range(n):
        for j in range(rp[i], rp[i + 1]):
            A[i, ci[j]] += va[j]
    return A
