"""NumPy restatement of the reference's BCSR rules, the yardstick of tests/test_gpu_bcsr.py.

  csr_to_bcsr   src/base/host/host_conversion.cpp:326-534
  bcsr_to_csr   src/base/host/host_conversion.cpp:537-579
  apply         HostMatrixBCSR::Apply     src/base/host/host_matrix_bcsr.cpp:330-377
  apply_add     HostMatrixBCSR::ApplyAdd  src/base/host/host_matrix_bcsr.cpp:380-429

Plain Python loops, one rounded operation at a time in the matrix' own precision (NumPy scalars of that dtype: a product
is rounded, then the sum is).  Values of a block are column-major: val[j * d * d + bi + bj * d].
"""
import numpy as np


def bcsr_ind(j, bi, bj, d):
    return j * d * d + bi + bj * d


def csr_to_bcsr(rp, ci, va, nrow, ncol, d):
    """-> (brp, bci, bval) or None where the reference refuses (nrow or ncol no multiple of d).  The block columns of a block
    row come out ascending (the reference collects them in order of appearance and sorts blocks and columns together
    afterwards); a column stored twice in a CSR row keeps the entry stored later."""
    assert d > 1
    if nrow % d != 0 or ncol % d != 0:
        return None
    va = np.asarray(va)
    mb = nrow // d
    brp = np.zeros(mb + 1, dtype=np.int32)
    cols_of = []
    for b in range(mb):
        seen = []
        for i in range(d):
            r = b * d + i
            for j in range(int(rp[r]), int(rp[r + 1])):
                bc = int(ci[j]) // d
                if bc not in seen:
                    seen.append(bc)
        seen.sort()
        cols_of.append(seen)
        brp[b + 1] = brp[b] + len(seen)
    nnzb = int(brp[mb])
    bci = np.zeros(nnzb, dtype=np.int32)
    bval = np.zeros(nnzb * d * d, dtype=va.dtype)
    for b in range(mb):
        where = {}
        for k, bc in enumerate(cols_of[b]):
            bci[brp[b] + k] = bc
            where[bc] = int(brp[b]) + k
        for i in range(d):
            r = b * d + i
            for j in range(int(rp[r]), int(rp[r + 1])):
                c = int(ci[j])
                bval[bcsr_ind(where[c // d], i, c % d, d)] = va[j]
    return brp, bci, bval


def bcsr_to_csr(brp, bci, bval, d):
    """-> (rp, ci, va): all d * d entries of every block, padded zeros included"""
    bval = np.asarray(bval)
    mb = len(brp) - 1
    nnz = int(brp[mb]) * d * d
    rp = np.zeros(mb * d + 1, dtype=np.int32)
    ci = np.zeros(nnz, dtype=np.int32)
    va = np.zeros(nnz, dtype=bval.dtype)
    idx = 0
    for i in range(mb):
        for r in range(d):
            row = i * d + r
            for k in range(int(brp[i]), int(brp[i + 1])):
                for c in range(d):
                    ci[idx] = d * int(bci[k]) + c
                    va[idx] = bval[bcsr_ind(k, r, c, d)]
                    idx += 1
            rp[row + 1] = rp[row] + (int(brp[i + 1]) - int(brp[i])) * d
    return rp, ci, va


def _row_sums(brp, bci, bval, d, x):
    bval = np.asarray(bval)
    T = bval.dtype.type
    x = np.asarray(x, dtype=bval.dtype)
    mb = len(brp) - 1
    out = np.zeros(mb * d, dtype=bval.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for ai in range(mb):
            for bi in range(d):
                s = T(0)
                for aj in range(int(brp[ai]), int(brp[ai + 1])):
                    col = int(bci[aj])
                    for bj in range(d):
                        p = T(bval[bcsr_ind(aj, bi, bj, d)] * x[d * col + bj])
                        s = T(s + p)
                out[ai * d + bi] = s
    return out


def apply(brp, bci, bval, d, x):
    return _row_sums(brp, bci, bval, d, x)


def apply_add(brp, bci, bval, d, x, scalar, y):
    """out += scalar * sum: the scalar in the matrix' precision, one rounded product, one rounded add"""
    s = _row_sums(brp, bci, bval, d, x)
    T = s.dtype.type
    y = np.array(y, dtype=s.dtype)
    for r in range(len(s)):
        y[r] = T(y[r] + T(T(scalar) * s[r]))
    return y


def dense(brp, bci, bval, d, ncol):
    mb = len(brp) - 1
    A = np.zeros((mb * d, ncol), dtype=np.asarray(bval).dtype)
    for i in range(mb):
        for k in range(int(brp[i]), int(brp[i + 1])):
            for r in range(d):
                for c in range(d):
                    A[i * d + r, d * int(bci[k]) + c] = bval[bcsr_ind(k, r, c, d)]
    return A


def csr_dense(rp, ci, va, nrow, ncol):
    A = np.zeros((nrow, ncol), dtype=np.asarray(va).dtype)
    for r in range(nrow):
        for j in range(int(rp[r]), int(rp[r + 1])):
            A[r, int(ci[j])] = va[j]
    return A
