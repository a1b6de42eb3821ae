"""DIA without a GPU: the names the format adds to the ABI, the Python and the C++ layer, and -- so that no case of
tests/test_gpu_dia.py can pass by skipping -- the oracle's verdict on every matrix that file generates: accepted under the
reference's rule num_diag <= 5 * (nnz / nrow), with the properties the GPU test relies on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dia_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_python_layer_names():
    import rocalution_amd as ra
    from rocalution_amd import capi
    assert ra.DIA == 5 and capi.DIA == 5
    assert capi.SIGNATURES["ramd_mat_dia_info"][1] == [capi.mat_t, capi.pi32]
    assert capi.SIGNATURES["ramd_mat_copy_dia_to_host"][1] == [capi.mat_t, capi.ptr, capi.ptr]
    for meth in ("ConvertToDIA", "dia_arrays"):
        assert hasattr(ra.LocalMatrix, meth)


def test_abi_exports_the_new_symbols():
    from rocalution_amd import capi
    lib = capi.load()  # (resolves every name of capi.SIGNATURES)
    for name in ("ramd_mat_dia_info", "ramd_mat_copy_dia_to_host"):
        assert getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "rocalution_amd.h")).read()
    assert "RAMD_DIA = 5" in hdr
    assert "int ramd_mat_dia_info(ramd_mat_t m, int* num_diag);" in hdr
    assert "int ramd_mat_copy_dia_to_host(ramd_mat_t m, int32_t* offset, void* val);" in hdr


def test_cpp_layer_compiles_with_convert_to_dia(tmp_path):
    """LocalMatrix::ConvertToDIA() and ConvertTo(DIA) of include/rocalution compile with the host compiler (no link)"""
    src = tmp_path / "dia_api.cpp"
    src.write_text("#include <rocalution/rocalution.hpp>\n"
                   "using namespace rocalution;\n"
                   "unsigned int f(LocalMatrix<double>& a, LocalMatrix<float>& b)\n"
                   "{\n"
                   "    a.ConvertToDIA();\n"
                   "    b.ConvertTo(DIA);\n"
                   "    void (LocalMatrix<double>::*p)(void) = &LocalMatrix<double>::ConvertToDIA;\n"
                   "    (void)p;\n"
                   "    static_assert(DIA == 5 && RAMD_DIA == 5, \"numbering of matrix_formats.hpp\");\n"
                   "    return a.GetFormat() == DIA ? 1u : 0u;\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", cases.NAMES)
def test_the_oracle_accepts_every_generated_case(oracle, name, dtype):
    rp, ci, va = cases.case(name)
    n = len(rp) - 1
    assert np.array_equal(va.astype(np.float32).astype(np.float64), va)  # exact in fp32
    dia = oracle.csr_to_dia(rp, ci, va.astype(dtype))
    assert dia is not None, "refused: %d entries on %d rows" % (len(va), n)
    off, dv = dia
    assert np.all(np.diff(off) > 0) and len(dv) == len(off) * n
    assert len(off) <= 5 * (len(va) // n)
    dense = np.zeros((n, n), dtype)
    for r in range(n):
        for j in range(rp[r], rp[r + 1]):
            dense[r, ci[j]] = va[j]  # (the entry stored later stays)
    for d, o in enumerate(off):
        for r in range(n):
            want = dense[r, r + o] if 0 <= r + o < n else 0.0
            assert dv[d * n + r] == want
    brp, bci, bva = oracle.dia_to_csr(n, off, dv)
    assert np.all(bva != 0)
    for r in range(n):
        assert np.all(np.diff(bci[brp[r]:brp[r + 1]]) > 0)


def test_what_the_cases_are_there_for(oracle):
    off = {name: oracle.csr_to_dia(*cases.case(name))[0].tolist() for name in cases.NAMES}
    assert off["tri_1"] == [0] and off["tri_1000"] == [-1, 0, 1]
    assert off["band40_130"] == list(range(-20, 20))
    assert off["far300_1000"] == [-300, 0, 300]
    assert off["corners_200"] == [-199, 0, 199]
    assert off["off3_only"] == [3]
    assert off["holes_64"] == [-1, 0, 5]
    # unsorted rows give what sorted rows give
    rp, ci, va = cases.banded(257, (-17, -2, -1, 0, 1, 2, 17), 8)
    srp, sci, sva = cases.case("shuffled_257")
    assert not np.array_equal(ci, sci)
    a, b = oracle.csr_to_dia(rp, ci, va), oracle.csr_to_dia(srp, sci, sva)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the duplicate: the later entry is the one in the DIA values
    rp, ci, va = cases.case("duplicate_65")
    o, dv = oracle.csr_to_dia(rp, ci, va)
    assert dv[1 * 65 + 5] == -2.5 and dv[2 * 65 + 40] == 3.25
    # off3_only without its doubled entries is refused: nnz / n = 0
    assert oracle.csr_to_dia(*cases.banded(100, (3,), 7)) is None
    # zeros: -0.0 keeps its sign in DIA and leaves on the way back, with the other zeros
    rp, ci, va = cases.case("zeros_64")
    o, dv = oracle.csr_to_dia(rp, ci, va)
    assert np.sum(np.signbit(dv) & (dv == 0)) == 1
    assert len(oracle.dia_to_csr(64, o, dv)[2]) == len(va) - 4
    # holes: NaN exactly where the host loop multiplies a padded zero with +-inf or reads x[0]
    rp, ci, va = cases.case("holes_64")
    o, dv = oracle.csr_to_dia(rp, ci, va)
    y = oracle.dia_apply(64, o, dv, cases.special_x(64))
    assert np.nonzero(np.isnan(y))[0].tolist() == [0, 1, 20, 30]


@pytest.mark.parametrize("name,accepted", [("gr3030", True), ("poisson8", True), ("lap2d7", True), ("lap27_6", True),
                                           ("rand300", False), ("rand300ell", False)])
def test_goldens_accepted_and_refused(oracle, name, accepted):
    g = load_golden(name)
    assert (int(g["dia_format"][0]) == oracle.DIA) == accepted
    assert (oracle.csr_to_dia(g["rowptr"], g["col"], g["val"].astype(np.float32)) is not None) == accepted  # fp32: the same verdict
