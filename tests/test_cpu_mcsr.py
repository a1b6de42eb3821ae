"""MCSR without a GPU: the names the format adds to the ABI, the Python and the C++ layer; tests/_mcsr_ref.py pinned byte for
byte to the genuine library's recorded results (tests/golden/mcsr, tools/gen_golden_mcsr.py); and its verdict on every matrix
tests/test_gpu_mcsr.py generates, so that no GPU case rests on an unchecked refusal."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mcsr_cases as cases  # noqa: E402
import _mcsr_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHIVES = ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300", "rand300ell", "shuffled_257", "longrow", "hub", "zeros_64",
            "negzero_64", "nodiag_row_40"]
DTYPES = [np.float64, np.float32]


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%d elements differ" % np.sum(a != b)


def test_python_layer_names():
    import rocalution_amd as ra
    from rocalution_amd import capi
    assert ra.MCSR == 2 and capi.MCSR == 2
    assert capi.SIGNATURES["ramd_mat_set_mcsr"][1] == [capi.mat_t, capi.i32, capi.i32, capi.i64, capi.ptr, capi.ptr, capi.ptr]
    assert capi.SIGNATURES["ramd_mat_copy_mcsr_to_host"][1] == [capi.mat_t, capi.ptr, capi.ptr, capi.ptr]
    for meth in ("ConvertToMCSR", "SetDataPtrMCSR", "mcsr_arrays"):
        assert hasattr(ra.LocalMatrix, meth)


def test_abi_exports_the_new_symbols():
    from rocalution_amd import capi
    lib = capi.load()  # (resolves every name of capi.SIGNATURES)
    for name in ("ramd_mat_set_mcsr", "ramd_mat_copy_mcsr_to_host"):
        assert getattr(lib, name) is not None
    hdr = open(os.path.join(ROOT, "include", "rocalution_amd.h")).read()
    assert "RAMD_MCSR = 2" in hdr and "MCSR = 2: not provided" not in hdr
    assert ("int ramd_mat_set_mcsr(ramd_mat_t m, int nrow, int ncol, int64_t nnz, const int32_t* row_offset, const int32_t* col, "
            "const void* val);") in hdr
    assert "int ramd_mat_copy_mcsr_to_host(ramd_mat_t m, int32_t* row_offset, int32_t* col, void* val);" in hdr


def test_cpp_layer_compiles_with_the_mcsr_entries(tmp_path):
    """ConvertToMCSR / ConvertTo(MCSR), AllocateMCSR, SetDataPtrMCSR and LeaveDataPtrMCSR of include/rocalution compile with the
    host compiler (no link); the C++ enum and the C enum agree on the number"""
    src = tmp_path / "mcsr_api.cpp"
    src.write_text("#include <rocalution/rocalution.hpp>\n"
                   "using namespace rocalution;\n"
                   "unsigned int f(LocalMatrix<double>& a, LocalMatrix<float>& b)\n"
                   "{\n"
                   "    a.ConvertToMCSR();\n"
                   "    b.ConvertTo(MCSR);\n"
                   "    void (LocalMatrix<double>::*p)(void) = &LocalMatrix<double>::ConvertToMCSR;\n"
                   "    (void)p;\n"
                   "    int *ro = NULL, *col = NULL;\n"
                   "    float* val = NULL;\n"
                   "    b.LeaveDataPtrMCSR(&ro, &col, &val);\n"
                   "    b.SetDataPtrMCSR(&ro, &col, &val, \"b\", 7, 3, 3);\n"
                   "    a.AllocateMCSR(\"a\", 10, 4, 4);\n"
                   "    static_assert(MCSR == 2 && RAMD_MCSR == 2, \"numbering of matrix_formats.hpp\");\n"
                   "    return a.GetFormat() == MCSR ? 1u : 0u;\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


# ----------------------------------------------------------------------------------------- the restatement against the library
@pytest.mark.parametrize("name", ARCHIVES)
def test_the_restatement_reproduces_every_array_of_every_archive(name):
    g = ref.load(name)
    assert sorted(n[:-4] for n in os.listdir(ref.GOLDEN)) == sorted(ARCHIVES)  # (no archive goes unchecked)
    rp, ci, x, y = g["rowptr"], g["col"], g["x"], g["y"]
    checked = {"rowptr", "col", "val", "x", "y", "format", "csr_differs", "rhs"}
    for dtype, sfx in ((np.float64, ""), (np.float32, "_f32")):
        va = g["val"].astype(dtype)
        m = ref.csr_to_mcsr(rp, ci, va)
        assert (m is not None) == (int(g["format"][0]) == 2)
        if m is None:
            continue
        ro, col, val = m
        eq(ro, g["mcsr_rowptr"]); eq(col, g["mcsr_col"]); eq(val, g["mcsr_val" + sfx])
        eq(ref.apply(ro, col, val, x), g["spmv_mcsr" + sfx])
        eq(ref.apply_add(ro, col, val, x, -0.75, y), g["spmv_mcsr_add" + sfx])
        brp, bci, bva = ref.mcsr_to_csr(ro, col, val)
        eq(brp, g["back_rowptr"]); eq(bci, g["back_col"]); eq(bva, g["back_val" + sfx])
        checked |= {"mcsr_rowptr", "mcsr_col", "mcsr_val" + sfx, "spmv_mcsr" + sfx, "spmv_mcsr_add" + sfx, "back_rowptr", "back_col",
                    "back_val" + sfx}
    assert set(g) - checked <= {"cg_jacobi_mcsr_meta", "cg_jacobi_mcsr_hist", "cg_jacobi_mcsr_x"}, set(g) - checked


@pytest.mark.parametrize("name", ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300", "rand300ell"])
def test_the_fixtures_are_the_committed_operators_and_round_trip_to_themselves(name):
    from conftest import load_golden
    g, base = ref.load(name), load_golden(name)
    eq(g["rowptr"], base["rowptr"].astype(np.int32)); eq(g["col"], base["col"].astype(np.int32)); eq(g["val"], base["val"])
    # sorted rows with a full diagonal come back byte for byte
    eq(g["back_rowptr"], g["rowptr"]); eq(g["back_col"], g["col"]); eq(g["back_val"], g["val"])
    assert int(g["mcsr_rowptr"][0]) == len(g["rowptr"]) - 1 and int(g["mcsr_rowptr"][-1]) == len(g["val"])
    assert not np.any(g["mcsr_col"][:len(g["rowptr"]) - 1])


@pytest.mark.parametrize("name", ["shuffled_257", "gr3030"])
def test_the_goldens_tell_the_two_summation_orders_apart(name):
    """spmv_mcsr differs from the CSR loop's sum of the same operands in at least one element, in both value types: otherwise a
    product that sums in CSR's order would pass.  Recorded counts (tools/gen_golden_mcsr.py): gr3030 195 of 900 rows in fp64 and
    275 in fp32, shuffled_257 69 and 71 of 257"""
    g = ref.load(name)
    counts = []
    for dtype, sfx, u in ((np.float64, "", np.uint64), (np.float32, "_f32", np.uint32)):
        c = ref.csr_apply(g["rowptr"], g["col"], g["val"].astype(dtype), g["x"].astype(dtype))
        counts.append(int(np.sum(c.view(u) != g["spmv_mcsr" + sfx].view(u))))
    print(name, counts)
    assert counts == g["csr_differs"].tolist() and min(counts) >= 1
    if name == "gr3030":  # ... and from the committed CSR product of the same x
        from conftest import load_golden
        base = load_golden(name)
        eq(g["x"], base["x"])
        assert np.sum(base["spmv_csr"] != g["spmv_mcsr"]) == counts[0]


# -------------------------------------------------------------------------------------------------------- the generated cases
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.ACCEPTED)
def test_the_restatement_accepts_every_case_meant_to_be_accepted(name, dtype):
    rp, ci, va = cases.case(name)
    n = len(rp) - 1
    assert cases.shape(name) == (n, n)
    assert np.array_equal(va.astype(np.float32).astype(np.float64), va) and np.all(np.abs(va) <= 8) and np.all(va * 8 == np.round(va * 8))
    m = ref.csr_to_mcsr(rp, ci, va.astype(dtype))
    assert m is not None
    ro, col, val = m
    assert ro[0] == n and ro[n] == len(va) and np.all(np.diff(ro) >= 0) and not np.any(col[:n])
    for r in range(n):
        cols = ci[rp[r]:rp[r + 1]]
        assert np.sum(cols == r) == 1  # exactly one stored diagonal entry: the reference is well defined
        eq(col[ro[r]:ro[r + 1]], cols[cols != r])
    brp, bci, bva = ref.mcsr_to_csr(ro, col, val)
    eq(brp, rp)
    for r in range(n):
        assert np.all(np.diff(bci[brp[r]:brp[r + 1]]) > 0)
        order = np.argsort(ci[rp[r]:rp[r + 1]], kind="stable") + rp[r]
        eq(bci[brp[r]:brp[r + 1]], ci[order]); eq(bva[brp[r]:brp[r + 1]], va[order].astype(dtype))


def test_the_restatement_refuses_the_two_cases_meant_to_be_refused():
    rp, ci, va = cases.case("nodiag_row_40")
    assert 17 not in ci[rp[17]:rp[18]] and all(r in ci[rp[r]:rp[r + 1]] for r in range(40) if r != 17)
    assert ref.csr_to_mcsr(rp, ci, va) is None and ref.csr_to_mcsr(rp, ci, va.astype(np.float32)) is None
    rp, ci, va = cases.case("rect_5x7")
    assert cases.shape("rect_5x7") == (5, 7) and len(rp) == 6 and ci.max() == 6
    assert ref.csr_to_mcsr(rp, ci, va, nrow=5, ncol=7) is None
    with pytest.raises(ValueError):  # a diagonal stored twice: outside what the restatement (and the reference) define
        ref.csr_to_mcsr(np.array([0, 2, 3], np.int32), np.array([0, 0, 1], np.int32), np.ones(3))


def test_what_the_cases_are_there_for():
    # shuffled_257: unsorted rows, the diagonal first, last and in the middle of a row
    rp, ci, va = cases.case("shuffled_257")
    where = set()
    for r in range(257):
        cols = ci[rp[r]:rp[r + 1]].tolist()
        k = cols.index(r)
        where.add("first" if k == 0 else "last" if k == len(cols) - 1 else "middle")
    assert where == {"first", "last", "middle"}
    assert any(np.any(np.diff(ci[rp[r]:rp[r + 1]]) < 0) for r in range(257))
    # longrow: one row beyond a staging pass; a wave beyond a pass without such a row
    rp, ci, va = cases.case("longrow")
    off = np.diff(rp) - 1
    assert off[70] > cases.CAP and off[64:128].sum() > cases.CAP
    assert off[128:192].max() < cases.CAP < off[128:192].sum()
    # hub: 514 entries in row 0, two to four in the rows beside it
    rp, ci, va = cases.case("hub")
    assert len(rp) - 1 == 2050 and rp[1] == 514 and set(np.diff(rp)[1:64].tolist()) <= {2, 3, 4}
    # diag_only_130: no off-diagonal entry at all
    ro = ref.csr_to_mcsr(*cases.case("diag_only_130"))[0]
    assert np.all(ro == 130)
    # zeros_64: zeros of both signs on and off the diagonal survive both conversions with their sign
    rp, ci, va = cases.case("zeros_64")
    ro, col, val = ref.csr_to_mcsr(rp, ci, va)
    zero = val == 0
    assert np.sum(zero[:64]) == 2 and np.sum(zero[64:]) == 4
    assert np.sum(np.signbit(val[:64]) & zero[:64]) == 1 and np.sum(np.signbit(val[64:]) & zero[64:]) == 2
    eq(ref.mcsr_to_csr(ro, col, val)[2], va)
    # negzero_64: -0.0 in rows 0 .. 31, where the CSR loop gives +0.0
    rp, ci, va = cases.case("negzero_64")
    x = cases.x_for("negzero_64")
    for dtype in DTYPES:
        y = ref.apply(*ref.csr_to_mcsr(rp, ci, va.astype(dtype)), x)
        c = ref.csr_apply(rp, ci, va.astype(dtype), x)
        assert np.all(y[:32] == 0) and np.all(np.signbit(y[:32])) and np.all(c[:32] == 0) and not np.any(np.signbit(c[:32]))
