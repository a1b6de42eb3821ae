"""BCSR without a GPU: the NumPy restatement of the reference's rules (tests/_bcsr_ref.py) against a hand-worked example and
the committed goldens, and the names the format adds to the Python layer."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bcsr_ref as ref  # noqa: E402


def test_hand_worked_4x6_blockdim_2():
    """      c0 c1 | c2 c3 | c4 c5
       r0 [  1  .  |  .  . |  2  . ]     block row 0: block columns 0, 2
       r1 [  .  3  |  .  . |  .  4 ]
       r2 [  .  . |  5  6 |  .  . ]     block row 1: block columns 1, 2
       r3 [  .  . |  .  7 |  8  . ]
    row 0 stores its columns in descending order: the block columns still come out ascending"""
    rp = np.array([0, 2, 4, 6, 8], np.int32)
    ci = np.array([4, 0, 1, 5, 2, 3, 3, 4], np.int32)
    va = np.array([2.0, 1.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, 4, 6, 2)
    assert brp.tolist() == [0, 2, 4]
    assert bci.tolist() == [0, 2, 1, 2]
    # column-major blocks: [a00 a10 a01 a11]
    assert bval.tolist() == [1, 0, 0, 3,  2, 0, 0, 4,  5, 0, 6, 7,  0, 8, 0, 0]
    rp2, ci2, va2 = ref.bcsr_to_csr(brp, bci, bval, 2)
    assert rp2.tolist() == [0, 4, 8, 12, 16]
    assert ci2.tolist() == [0, 1, 4, 5,  0, 1, 4, 5,  2, 3, 4, 5,  2, 3, 4, 5]
    assert va2.tolist() == [1, 0, 2, 0,  0, 3, 0, 4,  5, 6, 0, 0,  0, 7, 8, 0]
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert ref.apply(brp, bci, bval, 2, x).tolist() == [11.0, 30.0, 39.0, 68.0]
    y = np.array([1.0, 1.0, 1.0, 1.0])
    assert ref.apply_add(brp, bci, bval, 2, x, -0.5, y).tolist() == [-4.5, -14.0, -18.5, -33.0]
    assert ref.csr_to_bcsr(rp, ci, va, 4, 6, 3) is None and ref.csr_to_bcsr(rp, ci, va, 4, 6, 4) is None  # 4 % 3, 6 % 4


CASES = [("poisson8", 2), ("poisson8", 4), ("poisson8", 8), ("rand300", 2), ("rand300", 3), ("rand300", 5), ("rand300", 6),
         ("lap27_6", 2), ("lap27_6", 3), ("lap27_6", 4)]


@pytest.mark.parametrize("name,d", CASES)
def test_restatement_on_the_goldens(name, d):
    g = load_golden(name)
    rp, ci, va = g["rowptr"], g["col"], g["val"]
    n = len(rp) - 1
    brp, bci, bval = ref.csr_to_bcsr(rp, ci, va, n, n, d)
    for b in range(n // d):  # distinct and ascending
        assert np.all(np.diff(bci[brp[b]:brp[b + 1]]) > 0)
    D = ref.csr_dense(rp, ci, va, n, n)
    assert np.array_equal(ref.dense(brp, bci, bval, d, n), D)
    # the round trip adds explicit zeros and nothing else
    rp2, ci2, va2 = ref.bcsr_to_csr(brp, bci, bval, d)
    assert rp2[-1] == len(bci) * d * d == len(va2)
    assert np.array_equal(ref.csr_dense(rp2, ci2, va2, n, n), D)
    stored = np.zeros((n, n), bool)
    for r in range(n):
        stored[r, ci[rp[r]:rp[r + 1]]] = True
        assert np.all(np.diff(ci2[rp2[r]:rp2[r + 1]]) > 0)
        extra = ~stored[r, ci2[rp2[r]:rp2[r + 1]]]
        assert np.all(va2[rp2[r]:rp2[r + 1]][extra] == 0)
    # sorted CSR rows: the padded entries add +0, the product is the CSR product bit for bit
    rows_sorted = all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(n))
    if rows_sorted:
        assert np.array_equal(ref.apply(brp, bci, bval, d, g["x"]), g["spmv_csr"])
    else:
        assert np.allclose(ref.apply(brp, bci, bval, d, g["x"]), g["spmv_csr"], rtol=1e-12, atol=1e-12)


def test_at_least_two_goldens_have_sorted_rows():
    """(so the bit-for-bit leg above is not vacuous)"""
    k = 0
    for name in ("poisson8", "rand300", "lap27_6"):
        g = load_golden(name)
        rp, ci = g["rowptr"], g["col"]
        k += all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(len(rp) - 1))
    assert k >= 2


def test_python_layer_names():
    import rocalution_amd as ra
    from rocalution_amd import capi
    assert ra.BCSR == 3 and capi.BCSR == 3
    for name in ("ramd_mat_convert_bcsr", "ramd_mat_bcsr_info", "ramd_mat_copy_bcsr_to_host"):
        assert name in capi.SIGNATURES
    assert capi.SIGNATURES["ramd_mat_convert_bcsr"][1] == [capi.mat_t, capi.i32]
    for meth in ("ConvertToBCSR", "bcsr_arrays"):
        assert hasattr(ra.LocalMatrix, meth)
    import inspect
    assert "blockdim" in inspect.signature(ra.LocalMatrix.ConvertTo).parameters


def test_cpp_layer_has_the_reference_signatures(tmp_path):
    """LocalMatrix::ConvertTo(BCSR, blockdim) and ConvertToBCSR(int) of include/rocalution compile (host compiler, no link)"""
    import subprocess
    cxx = "g++"  # (the host compiler the driver tests of this suite use)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "bcsr_api.cpp"
    src.write_text("#include <rocalution/rocalution.hpp>\n"
                   "using namespace rocalution;\n"
                   "void f(LocalMatrix<double>& a, LocalMatrix<float>& b)\n"
                   "{\n"
                   "    a.ConvertTo(BCSR, 5);\n"
                   "    a.ConvertToBCSR(5);\n"
                   "    b.ConvertToBCSR(2);\n"
                   "    void (LocalMatrix<double>::*p)(int) = &LocalMatrix<double>::ConvertToBCSR;\n"
                   "    (void)p;\n"
                   "}\n")
    r = subprocess.run([cxx, "-std=c++14", "-fsyntax-only", "-I" + os.path.join(root, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
