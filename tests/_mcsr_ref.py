"""A numpy restatement of the reference's four host loops for the MCSR format, in the operator's value type, with plain Python
row loops in storage order: csr_to_mcsr / mcsr_to_csr (src/base/host/host_conversion.cpp:146-323) and HostMatrixMCSR::Apply /
ApplyAdd (src/base/host/host_matrix_mcsr.cpp:421-494).  It is the yardstick for the generated cases of tests/_mcsr_cases.py;
tests/test_cpu_mcsr.py pins it to the genuine library's recorded results (tests/golden/mcsr/*.npz) byte for byte.

Defined on the inputs on which the reference is: every row stores exactly one diagonal entry (accepted), or at least one row
stores none and no row stores two (refused).  A row with two diagonal entries raises: the library under test refuses it, the
reference runs its fill loop misaligned."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcsr")


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def csr_to_mcsr(rp, ci, va, nrow=None, ncol=None):
    """-> (row_offset, col, val), or None where the reference refuses (non-square, or a row without a diagonal entry)"""
    n = len(rp) - 1 if nrow is None else nrow
    if n != (n if ncol is None else ncol):
        return None
    nnz = len(va)
    ndiag = [sum(1 for j in range(rp[i], rp[i + 1]) if ci[j] == i) for i in range(n)]
    if any(k > 1 for k in ndiag):
        raise ValueError("a row stores its diagonal entry twice: the reference is not defined here")
    if nnz > 0 and sum(ndiag) != n:
        return None
    ro = np.zeros(n + 1, np.int32)
    col = np.zeros(nnz, np.int32)
    val = np.zeros(nnz, va.dtype)
    if nnz == 0:  # (LocalMatrix::ConvertTo on a matrix without entries: an empty matrix of the new format)
        return ro, col, val
    for i in range(n + 1):
        ro[i] = n + rp[i] - i
    for i in range(n):
        corr = i
        for j in range(rp[i], rp[i + 1]):
            if ci[j] != i:
                col[n + j - corr] = ci[j]
                val[n + j - corr] = va[j]
            else:
                val[i] = va[j]
                corr += 1
    return ro, col, val


def mcsr_to_csr(ro, col, val):
    n, nnz = len(ro) - 1, len(val)
    rp = np.zeros(n + 1, np.int32)
    ci = np.zeros(nnz, np.int32)
    va = np.zeros(nnz, val.dtype)
    if nnz == 0:
        return rp, ci, va
    for i in range(n + 1):
        rp[i] = ro[i] - n + i
    for i in range(n):
        for j in range(ro[i], ro[i + 1]):
            ci[j - n + i] = col[j]
            va[j - n + i] = val[j]
        d = ro[i + 1] - n + i
        ci[d] = i
        va[d] = val[i]
    for i in range(n):  # the bubble sort, swapping on strict >
        lo, hi = int(rp[i]), int(rp[i + 1])
        for _ in range(lo, hi):
            swapped = False
            for jj in range(lo, hi - 1):
                if ci[jj] > ci[jj + 1]:
                    ci[jj], ci[jj + 1] = ci[jj + 1], ci[jj]
                    va[jj], va[jj + 1] = va[jj + 1], va[jj]
                    swapped = True
            if not swapped:  # (the remaining sweeps of the reference change nothing)
                break
    return rp, ci, va


def apply(ro, col, val, x):
    n = len(ro) - 1
    T = val.dtype.type
    x = np.asarray(x, val.dtype)
    out = np.zeros(n, val.dtype)
    if len(val) == 0:
        return out
    with np.errstate(all="ignore"):
        for i in range(n):
            s = T(val[i] * x[i])
            for j in range(ro[i], ro[i + 1]):
                s = T(s + T(val[j] * x[col[j]]))
            out[i] = s
    return out


def apply_add(ro, col, val, x, scalar, y):
    n = len(ro) - 1
    T = val.dtype.type
    x = np.asarray(x, val.dtype)
    out = np.array(y, val.dtype)
    if len(val) == 0:
        return out
    sc = T(scalar)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = T(out[i] + T(T(sc * val[i]) * x[i]))
            for j in range(ro[i], ro[i + 1]):
                s = T(s + T(T(sc * val[j]) * x[col[j]]))
            out[i] = s
    return out


def csr_apply(rp, ci, va, x):
    """the CSR host loop (sum from zero, storage order) for comparison: what MCSR must NOT equal everywhere"""
    T = va.dtype.type
    x = np.asarray(x, va.dtype)
    out = np.zeros(len(rp) - 1, va.dtype)
    for i in range(len(rp) - 1):
        s = T(0)
        for j in range(rp[i], rp[i + 1]):
            s = T(s + T(va[j] * x[ci[j]]))
        out[i] = s
    return out
