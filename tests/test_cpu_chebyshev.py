"""CPU-side tests of the Chebyshev solver's surface: its number in the solver table, the two fused entries in header,
library and ctypes table, their signatures (vectors, scalars and slots only: the product between them is ramd_mat_apply,
which is how operators with 64-bit row offsets are served), and the drop-in compile of the C++ class."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rocalution_amd.h")
NEW_ENTRIES = ("ramd_fused_cheb_direction", "ramd_fused_cheb_residual")


def test_chebyshev_has_the_oracles_number(oracle):
    from rocalution_amd import capi, solvers
    assert capi.SOLVER_CHEBYSHEV == oracle.CHEBYSHEV == 10
    assert solvers.Chebyshev.kind == capi.SOLVER_CHEBYSHEV
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"\bRAMD_SOLVER_CHEBYSHEV\s*=\s*10\b", text)


def test_new_entries_in_header_library_and_ctypes_table():
    from rocalution_amd import build, capi
    lib = build.build()
    exported = set(re.findall(r" T (ramd_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()))
    declared = set(re.findall(r"\b(ramd_[a-z0-9_]+)\s*\(", open(HDR).read()))
    for name in NEW_ENTRIES:
        assert name in declared and name in exported and name in capi.SIGNATURES, name
    capi.load()


def _entries():
    """{entry: [(type, name), ...]} of the header, parsed as tests/test_gpu_wide_csr.py parses it"""
    h = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(ramd_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.S):
        params = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("", "void"):
                continue
            m = re.match(r"(.*?)(\w+)(?:\[\d*\])?$", a)
            params.append((m.group(1).strip(), m.group(2)))
        out[name] = params
    return out


def test_new_entries_take_no_matrix():
    entries = _entries()
    assert any(t == "ramd_mat_t" for t, _ in entries["ramd_fused_cg_update"] + entries["ramd_fused_apply_dot"])  # (the parser sees them)
    for name in NEW_ENTRIES:
        types = [t for t, _ in entries[name]]
        assert "ramd_mat_t" not in types and set(types) <= {"ramd_vec_t", "double", "int"}, (name, types)
    from rocalution_amd import capi
    assert len(capi.SIGNATURES["ramd_fused_cheb_direction"][1]) == len(entries["ramd_fused_cheb_direction"]) == 7
    assert len(capi.SIGNATURES["ramd_fused_cheb_residual"][1]) == len(entries["ramd_fused_cheb_residual"]) == 3


DRIVER = r"""
// Chebyshev as a reference driver uses it, for the three instantiations the library serves; plain host C++, no HIP headers
#include <rocalution/rocalution.hpp>
using namespace rocalution;
template <class Mat, class Vec, typename T>
void run(Mat& mat, Vec& rhs, Vec& x)
{
    Chebyshev<Mat, Vec, T> ls;
    Jacobi<Mat, Vec, T>    p;
    ls.Set((T)0.01, (T)2.0);
    ls.SetOperator(mat); ls.SetPreconditioner(p); ls.Init(1e-10, 1e-8, 1e8, 100); ls.SetFused(false);
    ls.Build(); ls.Print(); ls.Solve(rhs, &x); ls.ReBuildNumeric(); ls.Clear();
    Chebyshev<Mat, Vec, T> plain;
    plain.Set((T)0.05, (T)16.0); plain.SetOperator(mat); plain.Build(); plain.Solve(rhs, &x);
    (void)plain.GetIterationCount(); (void)plain.GetSolverStatus(); (void)plain.GetCurrentResidual();
    plain.Clear();
}
int main()
{
    init_rocalution();
    LocalMatrix<double> a; LocalVector<double> b, x;
    run<LocalMatrix<double>, LocalVector<double>, double>(a, b, x);
    LocalMatrix<float> af; LocalVector<float> bf, xf;
    run<LocalMatrix<float>, LocalVector<float>, float>(af, bf, xf);
    ParallelManager pm; GlobalMatrix<double> g(pm); GlobalVector<double> gb(pm), gx(pm);
    run<GlobalMatrix<double>, GlobalVector<double>, double>(g, gb, gx);
    stop_rocalution();
    return 0;
}
"""


def test_chebyshev_driver_compiles_with_plain_gxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "chebyshev_driver.cpp")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])


def test_global_chebyshev_driver_compiles_with_plain_gxx():
    """tests/drivers/global_chebyshev_driver.cpp (run by the GPU suite) is host C++"""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "global_chebyshev_driver.cpp")])
