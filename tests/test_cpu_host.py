"""CPU-side tests (no GPU): the C ABI surface, the C++ API layer's drop-in compile, and the host logic
of the row-block decomposition exercised with 2 gloo ranks."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rocalution_amd.h")


def _declared(offscope=False):
    """entry points the header declares; the blocks behind RAMD_WITH_OFFSCOPE (SPAI / FSAI / RS-AMG / Gershgorin: out of
    scope, not in the default build) only on request"""
    text = open(HDR).read()
    blocks = re.findall(r"#ifdef RAMD_WITH_OFFSCOPE.*?#endif", text, flags=re.S)
    if offscope:
        text = "\n".join(blocks)
    else:
        for b in blocks:
            text = text.replace(b, "")
    return set(re.findall(r"\b(ramd_[a-z0-9_]+)\s*\(", text)) - {"ramd_exchange_cb", "ramd_allreduce_cb"}


def test_abi_header_library_and_ctypes_table_agree():
    from rocalution_amd import build, capi
    lib = build.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    exported = set(re.findall(r" T (ramd_[a-z0-9_]+)", out))
    declared, optional = _declared(), _declared(offscope=True)
    assert set(capi.OPTIONAL) == optional and not (optional & declared)
    if exported & optional:  # a library built with -DRAMD_WITH_OFFSCOPE exports all of them
        assert optional <= exported
        exported -= optional
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert set(capi.SIGNATURES) == declared
    capi.load()  # dlopen + every prototype attached


def test_library_refuses_to_run_without_a_gpu():
    from rocalution_amd import capi
    lib = capi.load()
    import ctypes as C
    c = C.c_int(0)
    lib.ramd_device_count(C.byref(c))
    if c.value > 0:
        pytest.skip("a GPU is present")
    assert lib.ramd_init(-1) == capi.ERR_NO_DEVICE
    assert b"no host compute path" in lib.ramd_last_error()
    import rocalution_amd as ra
    with pytest.raises(ra.RamdError):
        ra.LocalVector()  # no silent CPU fallback anywhere


DRIVER = r"""
// a driver written against the reference API (cf. clients/samples/cg.cpp, gmres.cpp, bicgstab.cpp,
// mixed-precision.cpp, cg_mpi.cpp) -- must compile with a plain host compiler, no HIP headers
#include <rocalution/rocalution.hpp>
using namespace rocalution;
int main(int argc, char** argv)
{
    init_rocalution();
    info_rocalution();
    LocalVector<double> x, rhs, e;
    LocalMatrix<double> mat;
    mat.ReadFileMTX(std::string(argv[1]));
    mat.MoveToAccelerator(); x.MoveToAccelerator(); rhs.MoveToAccelerator(); e.MoveToAccelerator();
    x.Allocate("x", mat.GetN()); rhs.Allocate("rhs", mat.GetM()); e.Allocate("e", mat.GetN());
    CG<LocalMatrix<double>, LocalVector<double>, double> ls;
    Jacobi<LocalMatrix<double>, LocalVector<double>, double> p;
    e.Ones(); mat.Apply(e, &rhs); x.Zeros();
    ls.SetOperator(mat); ls.SetPreconditioner(p); ls.Build(); ls.Verbose(1);
    mat.Info();
    double tick = rocalution_time();
    ls.Solve(rhs, &x);
    double tack = rocalution_time();
    std::cout << "Solver execution:" << (tack - tick) / 1e6 << " sec" << std::endl;
    ls.Clear();
    GMRES<LocalMatrix<double>, LocalVector<double>, double> gm;
    ILU<LocalMatrix<double>, LocalVector<double>, double> ilu;
    gm.SetOperator(mat); gm.SetBasisSize(30); gm.SetPreconditioner(ilu); gm.Build(); x.Zeros(); gm.Solve(rhs, &x); gm.Clear();
    BiCGStab<LocalMatrix<double>, LocalVector<double>, double> bi;
    MultiColoredSGS<LocalMatrix<double>, LocalVector<double>, double> sgs;
    bi.SetOperator(mat); bi.SetPreconditioner(sgs); bi.Build(); mat.ConvertToELL(); x.Zeros(); bi.Solve(rhs, &x); bi.Clear();
    MixedPrecisionDC<LocalMatrix<double>, LocalVector<double>, double, LocalMatrix<float>, LocalVector<float>, float> mp;
    CG<LocalMatrix<float>, LocalVector<float>, float> cgf;
    cgf.Init(1e-5, 1e-2, 1e+20, 100000);
    mat.ConvertToCSR(); mp.SetOperator(mat); mp.Set(cgf); mp.Build(); x.Zeros(); mp.Solve(rhs, &x); mp.Clear();
    ParallelManager pm; GlobalMatrix<double> gmat(pm); GlobalVector<double> gx(pm), grhs(pm);
    CG<GlobalMatrix<double>, GlobalVector<double>, double> gls;
    BlockJacobi<GlobalMatrix<double>, GlobalVector<double>, double> bj;
    bj.Set(sgs); gls.SetOperator(gmat); gls.SetPreconditioner(bj);
    // the remaining Krylov drivers / multi-coloured preconditioners, Local and Global instantiations
    FCG<LocalMatrix<double>, LocalVector<double>, double> fcg; fcg.SetOperator(mat);
    CR<LocalMatrix<double>, LocalVector<double>, double> cr; cr.SetOperator(mat);
    FGMRES<LocalMatrix<double>, LocalVector<double>, double> fg; fg.SetBasisSize(20); fg.SetOperator(mat);
    BiCGStabl<LocalMatrix<double>, LocalVector<double>, double> bl; bl.SetOrder(4); bl.SetOperator(mat);
    QMRCGStab<LocalMatrix<double>, LocalVector<double>, double> qm; qm.SetOperator(mat);
    MultiColoredGS<LocalMatrix<double>, LocalVector<double>, double> mgs;
    MultiColoredILU<LocalMatrix<double>, LocalVector<double>, double> milu; milu.Set(0);
    qm.SetPreconditioner(mgs); fg.SetPreconditioner(milu);
    FCG<GlobalMatrix<double>, GlobalVector<double>, double> gfcg; gfcg.SetOperator(gmat);
    CR<GlobalMatrix<double>, GlobalVector<double>, double> gcr; gcr.SetOperator(gmat);
    FGMRES<GlobalMatrix<double>, GlobalVector<double>, double> gfg; gfg.SetOperator(gmat);
    BiCGStabl<GlobalMatrix<double>, GlobalVector<double>, double> gbl; gbl.SetOperator(gmat);
    QMRCGStab<GlobalMatrix<double>, GlobalVector<double>, double> gqm; gqm.SetOperator(gmat);
    IDR<LocalMatrix<double>, LocalVector<double>, double> idr; idr.SetOperator(mat); idr.SetShadowSpace(4); idr.SetRandomSeed(7ULL);
    IDR<GlobalMatrix<double>, GlobalVector<double>, double> gidr; gidr.SetOperator(gmat);
    x.SetRandomUniform(12345ULL, -4.0, 6.0);
    mat.WriteFileMTX("a.mtx"); mat.WriteFileCSR("a.csr"); mat.ReadFileCSR("a.csr");
    x.WriteFileASCII("x.dat"); x.ReadFileBinary("x.bin");
    e.ScaleAdd(-1.0, x);
    std::cout << "||e - x||_2 = " << e.Norm() << std::endl;
    stop_rocalution();
    return 0;
}
"""


def test_reference_style_driver_compiles_with_plain_gxx():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "driver.cpp")
        open(src, "w").write(DRIVER)
        subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), src])


def test_partition_csr_host_driver(tmp_path):
    """include/rocalution/distribute.hpp: the row-block split of a replicated matrix (clients/include/common.hpp:56-431) is
    pure host arithmetic -- tests/drivers/partition_driver.cpp checks it for 1..7 ranks: block rule, send list of r for q ==
    receive list of q from r, distributed product == A x, and on a symmetric pattern the reference's own-rows construction"""
    from rocalution_amd import build as B
    B.build()
    exe = str(tmp_path / "partition_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "partition_driver.cpp"), "-o", exe, "-L" + libdir,
                           "-lrocalution_amd", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"partition_driver ok" in r.stdout, r.stdout.decode()[-1500:]
    # the same pieces as rocalution_amd/distributed.py builds (the implementation the 2-rank runs exercise)
    from rocalution_amd import distributed as D
    nx, ny = 7, 9
    rows, cols, vals = [], [], []
    for j in range(ny):
        for i in range(nx):
            k = j * nx + i
            for ok, c, v in ((j > 0, k - nx, -1), (i > 0, k - 1, -2), (True, k, 9), (i < nx - 1, k + 1, -3), (j < ny - 1, k + nx, -4)):
                if ok:
                    rows.append(k); cols.append(c); vals.append(float(v))
    n = nx * ny
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int32)
    ci, va = np.asarray(cols, np.int32), np.asarray(vals)
    for ranks in (1, 2, 3, 5):
        out = subprocess.run([exe, "dump", str(ranks)], stdout=subprocess.PIPE, timeout=60, check=True).stdout.decode().splitlines()
        assert len(out) == ranks
        off = D.partition_rows(n, ranks)
        pieces = [D.split_rows(rp, ci, va, off, r) for r in range(ranks)]
        needs = []
        for pc in pieces:
            needs.append({int(p): pc["recv_global"][pc["recv_offset"][k]:pc["recv_offset"][k + 1]] for k, p in enumerate(pc["recv_peers"])})
        for r, line in enumerate(out):
            f = dict(kv.split("=") for kv in line.split())
            lst = lambda key: [int(t) for t in f[key].split(",")] if f[key] else []
            plan = D.build_halo_plan(pieces[r], off, r, lambda obj: needs)
            assert int(f["rank"]) == r
            assert lst("peers") == [int(p) for p in plan["peers"]]
            assert lst("recv_offset") == [int(v) for v in plan["recv_offset"]] and lst("send_offset") == [int(v) for v in plan["send_offset"]]
            assert lst("boundary") == [int(v) for v in plan["boundary_index"]]
            (irp, ici, iva), (grp, gci, gva) = pieces[r]["interior"], pieces[r]["ghost"]
            assert lst("int_rp") == irp.tolist() and lst("int_col") == ici.tolist() and lst("int_val") == [int(v) for v in iva]
            assert lst("gst_rp") == grp.tolist() and lst("gst_col") == gci.tolist() and lst("gst_val") == [int(v) for v in gva]


def test_distribute_driver_compiles_with_plain_gxx():
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "distribute_driver.cpp")])


def test_parallel_manager_io_driver_compiles_with_plain_gxx():
    """tests/drivers/pm_io_driver.cpp (run by the GPU suite: a communicator needs an initialised device) is host C++"""
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "pm_io_driver.cpp")])


@pytest.mark.parametrize("sample", ["samples/krylov_driver.cpp", "tests/drivers/multigrid_driver.cpp"])
def test_sample_drivers_compile_with_plain_gxx(sample):
    """the C++ drivers (run end to end by the GPU suite) are plain host C++ on include/rocalution: no hipcc, no device"""
    subprocess.check_call(["g++", "-std=c++14", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, *sample.split("/"))])


def test_partition_matches_reference_rule():
    from rocalution_amd import distributed as D
    for n, p in ((10, 3), (900, 2), (7, 8), (512 ** 3, 8)):
        off = D.partition_rows(n, p)
        sizes = np.diff(off)
        assert off[0] == 0 and off[-1] == n and sizes.max() - sizes.min() <= 1
        assert np.all(sizes[: n % p] == n // p + 1)  # the first nrow % P ranks get one more row


def test_split_rows_and_halo_plan_single_process():
    """assemble all ranks' pieces in one process and check y = A x piecewise"""
    from rocalution_amd import distributed as D, generators as gen
    rp, ci, va = gen.poisson7(6)
    n = len(rp) - 1
    import scipy.sparse as sp
    A = sp.csr_matrix((va, ci, rp), shape=(n, n))
    x = np.random.default_rng(0).uniform(-1, 1, n)
    for world in (1, 2, 3, 5):
        off = D.partition_rows(n, world)
        pieces = [D.split_rows(rp, ci, va, off, r) for r in range(world)]
        needs = [{int(p): pc["recv_global"][pc["recv_offset"][k]:pc["recv_offset"][k + 1]]
                  for k, p in enumerate(pc["recv_peers"])} for pc in pieces]
        for r, pc in enumerate(pieces):
            plan = D.build_halo_plan(pc, off, r, lambda obj: needs)
            lo, hi = pc["row_begin"], pc["row_end"]
            irp, ici, iva = pc["interior"]
            grp, gci, gva = pc["ghost"]
            recv = x[pc["recv_global"]]
            y = sp.csr_matrix((iva, ici, irp), shape=(hi - lo, hi - lo)) @ x[lo:hi]
            if len(gva):
                y = y + sp.csr_matrix((gva, gci, grp), shape=(hi - lo, len(recv))) @ recv
            assert np.allclose(y, (A @ x)[lo:hi], rtol=1e-14, atol=1e-14)
            # what I send is what my neighbours expect to receive, in their order
            for k, q in enumerate(plan["peers"]):
                mine = plan["boundary_index"][plan["send_offset"][k]:plan["send_offset"][k + 1]] + lo
                assert np.array_equal(mine, needs[int(q)][r])


def _spawn(mode, kind, world=2, timeout=300, env=None):
    with tempfile.TemporaryDirectory() as d:
        initfile = os.path.join(d, "init")
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_dist_worker.py"), mode, str(r),
                                   str(world), initfile, kind, d], env=dict(os.environ, **(env or {}))) for r in range(world)]
        for p in procs:
            assert p.wait(timeout=timeout) == 0
        return [dict(np.load(os.path.join(d, "r%d.npz" % r))) for r in range(world)]


@pytest.mark.parametrize("kind", ["poisson", "gr3030", "random", "lap27"])
def test_two_rank_gloo_spmv_and_cg_match_single_rank(kind, oracle):
    """world_size-2 gloo run of the decomposition (product host logic + oracle kernels) == 1-rank oracle"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _dist_worker as W
    rp, ci, va = W._matrix(kind)
    if kind == "random":
        rp, ci, va = W._symmetrize_pattern(rp, ci, va)
    n = len(rp) - 1
    x = np.random.default_rng(5).uniform(-1, 1, n)
    yref = oracle.csr_apply(rp, ci, va, x)
    b = oracle.csr_apply(rp, ci, va, np.ones(n))
    ref = oracle.solve(rp, ci, va, b, solver=oracle.CG, precond=oracle.PC_JACOBI, max_iter=500)
    res = _spawn("cpu", kind)
    y = np.concatenate([r["y"] for r in res])
    xs = np.concatenate([r["xs"] for r in res])
    assert np.allclose(y, yref, rtol=1e-13, atol=1e-13)
    assert abs(int(res[0]["it"]) - ref["iters"]) <= 1
    assert np.linalg.norm(xs - ref["x"]) / np.linalg.norm(ref["x"]) < 1e-8


# ------------------------------------------------------------------ file formats
def _parse_csr_file(path):
    """the reference's binary CSR layout (src/base/host/host_io.cpp:497-609)"""
    raw = open(path, "rb").read()
    head = b"#rocALUTION binary csr file\n"
    assert raw.startswith(head)
    o = len(head)
    version = int(np.frombuffer(raw, np.int32, 1, o)[0]); o += 4
    nrow, ncol, nnz = (int(v) for v in np.frombuffer(raw, np.int64, 3, o)); o += 24
    rp = np.frombuffer(raw, np.int32, nrow + 1, o); o += 4 * (nrow + 1)
    ci = np.frombuffer(raw, np.int32, nnz, o); o += 4 * nnz
    va = np.frombuffer(raw, np.float64, nnz, o); o += 8 * nnz
    assert o == len(raw)
    return version, nrow, ncol, rp, ci, va


def _same_but_version(a, b, header):
    """binary files carry the writer's version right after the header line"""
    ra, rb = open(a, "rb").read(), open(b, "rb").read()
    o = len(header)
    assert ra[:o] == rb[:o] == header
    assert ra[o + 4:] == rb[o + 4:]


def test_file_io_matches_reference_files(tmp_path):
    """read what the genuine library wrote, write it again: same bytes (binary: except the version
    stamp); MatrixMarket symmetric / pattern / unsorted general files give the reference's CSR"""
    import subprocess
    from rocalution_amd import build as B
    B.build()
    gold = os.path.join(ROOT, "tests", "golden", "io")
    exe = str(tmp_path / "io_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "io_driver.cpp"), "-o", exe,
                           "-L", libdir, "-lrocalution_amd", "-Wl,-rpath," + libdir])
    out = tmp_path / "out"; out.mkdir()
    r = subprocess.run([exe, gold, str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0, r.stdout.decode()
    exp = np.load(os.path.join(gold, "io_expected.npz"))
    ref_mtx = open(os.path.join(gold, "ref_A.mtx"), "rb").read()
    assert open(out / "A_from_mtx.mtx", "rb").read() == ref_mtx
    assert open(out / "A_from_csr.mtx", "rb").read() == ref_mtx
    head = b"#rocALUTION binary csr file\n"
    _same_but_version(str(out / "A_from_csr.csr"), os.path.join(gold, "ref_A.csr"), head)
    vf = _parse_csr_file(str(out / "A_float.csr"))  # fp32 matrix: values still stored as double
    assert np.array_equal(vf[5], exp["val"].astype(np.float32).astype(np.float64))
    v, nr, nc, rp, ci, va = _parse_csr_file(str(out / "A_from_csr.csr"))
    assert (nr, nc) == (25, 25) and v == 30200
    assert np.array_equal(rp, exp["rowptr"]) and np.array_equal(ci, exp["col"]) and np.array_equal(va, exp["val"])
    # the MatrixMarket text carries 12 significant digits
    v, nr, nc, rp, ci, va = _parse_csr_file(str(out / "A_from_mtx.csr"))
    assert np.array_equal(rp, exp["rowptr"]) and np.array_equal(ci, exp["col"])
    assert np.allclose(va, exp["val"], rtol=1e-11, atol=0)
    for nm in ("sym", "pat", "gen"):
        v, nr, nc, rp, ci, va = _parse_csr_file(str(out / ("read_%s.csr" % nm)))
        assert [nr, nc] == exp["read_%s_dims" % nm].tolist()
        assert np.array_equal(rp, exp["read_%s_rowptr" % nm])
        assert np.array_equal(ci, exp["read_%s_col" % nm])
        assert np.array_equal(va, exp["read_%s_val" % nm])
    ref_dat = open(os.path.join(gold, "ref_x.dat"), "rb").read()
    assert open(out / "x_from_ascii.dat", "rb").read() == ref_dat
    assert open(out / "x_from_bin.dat", "rb").read() == ref_dat
    _same_but_version(str(out / "x_from_bin.bin"), os.path.join(gold, "ref_x.bin"), b"#rocALUTION binary vector file\n")


def test_host_side_matrix_api(tmp_path):
    """COO input with the reference's ownership rules, Check(), LeaveDataPtrCOO, UpdateValuesCSR on host
    storage: a plain g++ program linked against the library, no accelerator needed"""
    import subprocess
    from rocalution_amd import build as B
    B.build()
    exe = str(tmp_path / "api_driver")
    libdir = os.path.join(ROOT, "rocalution_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "drivers", "api_driver.cpp"), "-o", exe,
                           "-L", libdir, "-lrocalution_amd", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"api_driver ok" in r.stdout, (r.returncode, r.stdout.decode()[-1500:])


def test_shell_surrogate_is_an_af_shell10_class_matrix(oracle, tmp_path):
    """config 3's stand-in: symmetric, positive definite (Gershgorin-free check through CG convergence), 5-unknown
    blocks, 25..45 entries per interior row, sorted rows; the symmetric MatrixMarket writer keeps the lower triangle"""
    from rocalution_amd import generators as gen
    rp, ci, va = gen.shell_surrogate(24, 20)
    n = len(rp) - 1
    assert n == 24 * 20 * 5
    A = gen.to_scipy(rp, ci, va)
    assert abs(A - A.T).max() == 0.0
    d = np.diff(rp)
    assert d.max() == 45 and d.min() >= 15 and 30.0 < d.mean() < 36.0
    assert all(np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0) for r in range(n))
    assert np.all(va * 128 == np.round(va * 128))  # exact binary fractions: no dependence on summation order
    # node degrees vary (irregular triangulation): not all interior rows have the same length
    assert len(set(d.tolist())) >= 4
    b = oracle.csr_apply(rp, ci, va, np.ones(n))
    r = oracle.solve(rp, ci, va, b, solver=oracle.CG, precond=oracle.PC_JACOBI, max_iter=5000)
    assert r["status"] == 2 and np.linalg.norm(r["x"] - 1.0) < 1e-3 * np.sqrt(n)  # SPD: CG converges
    path = str(tmp_path / "s.mtx")
    stored = gen.write_mtx_symmetric(path, rp, ci, va)
    assert stored == (len(ci) + n) // 2
    with open(path) as f:
        assert f.readline().strip() == "%%MatrixMarket matrix coordinate real symmetric"
        assert f.readline().split() == [str(n), str(n), str(stored)]
        rows = np.loadtxt(f)
    assert rows.shape == (stored, 3) and np.all(rows[:, 1] <= rows[:, 0])
    import scipy.sparse as sp
    L = sp.coo_matrix((rows[:, 2], (rows[:, 0].astype(int) - 1, rows[:, 1].astype(int) - 1)), shape=(n, n)).tocsr()
    full = L + sp.tril(L, -1).T
    assert abs(full - A).max() == 0.0


def test_bench_never_runs_on_fewer_ranks_than_asked():
    """`python bench.py --gpus 2` spawns its own ranks; without 2 devices it must fail loudly, not report 1 rank"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 2
    assert "need 2 devices" in p.stderr and p.stdout.strip() == ""


def test_bench_dump_sample_is_fixed_and_bounded():
    """bench.py --dump-outputs: an x of up to DUMP_ROWS rows is written whole; a longer one as the same seeded rows in every
    run (distinct, in order), DUMP_ROWS of them"""
    import bench

    class Vec:
        def __init__(self, n):
            self.v = np.arange(n, dtype=np.float64)

        def CopyToHostData(self):
            return self.v.copy()

    assert np.array_equal(bench.x_sample(Vec(1000)), np.arange(1000))
    n = 3 * bench.DUMP_ROWS
    a, b = bench.x_sample(Vec(n)), bench.x_sample(Vec(n))
    assert np.array_equal(a, b) and a.size == bench.DUMP_ROWS
    assert np.all(np.diff(a) > 0) and a[-1] < n and a.size * 8 <= 64 << 20


def test_blocked_mgs_recurrence_numpy_model():
    """the algebra behind ramd_fused_mgs_block (include/rocalution_amd.h; GMRES::doFusedMGS): with e_m = <v_m, w> and the
    block's Gram entries g_km = <v_k, v_m> taken in ONE pass over the un-updated w, forward substitution
    h_m = e_m - sum_{k<m} h_k g_km gives the modified Gram-Schmidt coefficients -- for an oblique basis too (the Gram
    entries are measured, not assumed zero).  numpy model of the device passes, blocks of 4, against the sequential loop."""
    import numpy as np
    rng = np.random.default_rng(11)
    n, m, K = 5000, 11, 4
    for oblique in (False, True):
        V = rng.uniform(-1, 1, (n, m))
        V = V / np.linalg.norm(V, axis=0) if oblique else np.linalg.qr(V)[0]
        w0 = rng.uniform(-1, 1, n)
        w = w0.copy(); href = np.zeros(m)
        for k in range(m):  # gmres.cpp:480-486
            href[k] = V[:, k] @ w
            w = w - href[k] * V[:, k]
        wb = w0.copy(); h = np.zeros(m); prev = None
        for b in range(0, m, K):
            blk = list(range(b, min(b + K, m)))
            if prev is not None:  # prologue of the pass: solve the previous block, apply it in MGS order
                for k in prev[0]:
                    wb = wb - h[k] * V[:, k]
            e = np.array([V[:, k] @ wb for k in blk])
            G = np.array([[V[:, a] @ V[:, c] for c in blk] for a in blk])
            for i, k in enumerate(blk):
                h[k] = e[i] - sum(h[blk[j]] * G[j, i] for j in range(i))
            prev = (blk,)
        for k in prev[0]:
            wb = wb - h[k] * V[:, k]
        tol = (1e-13 if not oblique else 2e-12) * np.linalg.norm(w0)
        assert np.max(np.abs(h - href)) <= tol
        assert np.max(np.abs(wb - w)) <= tol


# ------------------------------------------------------------------ the hand-off forms of the single-launch reductions
def test_grid_reduction_hand_off_is_emitted_in_the_write_through_forms(tmp_path):
    """Every dot / norm of every solver ends in grid_reduce_finish (csrc/device_utils.hpp): per-workgroup partials handed to the
    last workgroup WITHOUT a release fence -- 8-byte agent-scope atomics on both sides, the stores' completion before the
    ticket.  That is valid only in the forms the ISA gives those operations (MI355X_MICROARCH.md, "Workgroup dispatch, XCD
    placement & inter-workgroup visibility"): the partial's store write-through (`global_store ... sc1`), `s_waitcnt vmcnt(0)`
    between it and the ticket's atomic, the last workgroup's loads L1-bypassing (`global_load ... sc1`) behind an acquire
    (`buffer_inv sc1`).  The kernel's source is compiled for gfx950 with the library's flags and the assembly checked, so a
    compiler that lowers these operations differently fails here and not as a wrong residual norm under load."""
    import re
    import shutil
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = tmp_path / "probe.hip"
    src.write_text('''
#include "device_utils.hpp"
namespace ramd {
__global__ __launch_bounds__(kBlock) void k_probe_reduce(int64_t n, const double* __restrict__ a, ReduceCtx ctx, int slot)
{
    __shared__ double lds[8];
    double acc = 0.0;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        acc += a[i];
    const double vals[1] = {acc};
    const int slots[1] = {slot};
    const int ops[1] = {RED_SUM};
    grid_reduce_finish<1>(ctx, vals, slots, ops, lds);
}
}
''')
    out = tmp_path / "probe.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rocalution_amd", "csrc"),
           "--cuda-device-only", "-S", str(src), "-o", str(out)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:]
    body = out.read_text()
    body = body[body.index("k_probe_reduce"):]
    ops = [l.strip() for l in body.splitlines() if re.match(r"\s*(global_|buffer_|s_waitcnt vmcnt|s_barrier)", l)]
    st = [i for i, l in enumerate(ops) if l.startswith("global_store_dwordx2") and l.endswith("sc1")]
    at = [i for i, l in enumerate(ops) if l.startswith("global_atomic_add")]
    assert st and at and st[0] < at[0], ops
    # the partial is stored write-through, and the store has completed before the ticket is taken
    assert any(l.startswith("s_waitcnt vmcnt(0)") for l in ops[st[0] + 1:at[0]]), ops
    # the last workgroup: acquire, then loads that bypass the L1
    inv = [i for i, l in enumerate(ops) if l.startswith("buffer_inv") and "sc1" in l]
    assert inv and inv[0] > at[0], ops
    assert any(l.startswith("global_load_dwordx2") and l.endswith("sc1") for l in ops[inv[0]:]), ops
    # ... and nowhere a release fence (write-back of the XCD L2) per workgroup
    assert not any(l.startswith("buffer_wbl2") for l in ops), ops


# ------------------------------------------------------------------ the hand-counted waits of the lattice triangular solve
def test_lattice_solve_kernels_have_no_memory_operation_the_counts_do_not_know(tmp_path):
    """k_trsv_lat (csrc/trsv_lattice.hip) issues every vector memory operation of its pencil loop by hand and waits for loads by
    COUNTING the operations issued since (LatSched computes the counts at compile time).  That is valid only while the compiler
    adds no vector memory operation of its own inside the loop -- a register spill to scratch -- and never copies a register
    whose load is still in flight (values parked in accumulation registers above 256 VGPRs did exactly that: NaNs).  The file
    is compiled for gfx950 with the library's flags and every instantiation checked: no scratch, no spills, no v_accvgpr
    moves, at most 256 VGPRs; and the waits in front of the steps are the counts the schedule model predicts, not drains."""
    import re
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "lat.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rocalution_amd", "csrc"),
           "--cuda-device-only", "-S", os.path.join(ROOT, "rocalution_amd", "csrc", "trsv_lattice.hip"), "-o", str(out)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kern = re.findall(r"\.name:\s+(\S*k_trsv_lat\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)",
                      meta, flags=re.S)
    assert len(kern) == 16, [k[0] for k in kern]  # {fp64, fp32} x {lower, upper} x {unit, divide} x {16-byte, 8-byte staging}
    for name, scratch, vgpr, spill in kern:
        assert int(scratch) == 0 and int(spill) == 0 and int(vgpr) <= 256, (name, scratch, vgpr, spill)
    for name, _, _, _ in kern:
        start = text.index("\n" + name + ":")
        body = text[start:text.index("s_endpgm", start)]
        assert "v_accvgpr" not in body and "scratch_" not in body and "buffer_store" not in body, name
        waits = [int(w) for w in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)]
        # drains: the prologue / epilogue of a pencil and the re-poll loops of the 8 face batches of a loop body, nothing else
        assert sum(1 for w in waits if w == 0) <= 2 + 8 + 2, (name, waits)
        assert sum(1 for w in waits if w > 0) >= 16 + 2 + 8, (name, waits)


def test_pencil_solve_of_the_27_point_stencil_counts_its_own_waits(tmp_path):
    """k_trsv_box (csrc/trsv_box27.hip) does what k_trsv_lat does: loads and stores by hand, waits by count (box_wait<N>, N = the
    operations of a block less the step's own).  The counts hold only if the compiler adds no vector memory operation inside the
    block loop and copies no register whose load is in flight: all eight instantiations without scratch, spills or v_accvgpr; the
    four counted waits of a block are the ones the constants in the kernel give (35 / 33 for the steps, 40 for the polls); every hand-written 16-byte store is followed by two wait states (`s_nop 1`: the gfx950 hazard of round 6)."""
    import re
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "box.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rocalution_amd", "csrc"),
           "--cuda-device-only", "-S", os.path.join(ROOT, "rocalution_amd", "csrc", "trsv_box27.hip"), "-o", str(out)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kern = re.findall(r"\.name:\s+(\S*k_trsv_box\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)",
                      meta, flags=re.S)
    assert len(kern) == 8, [k[0] for k in kern]  # {fp64, fp32} x {lower, upper} x {unit, divide}
    for name, scratch, vgpr, spill in kern:
        assert int(scratch) == 0 and int(spill) == 0 and int(vgpr) <= 256, (name, scratch, vgpr, spill)
        start = text.index("\n" + name + ":")
        body = text[start:text.index("s_endpgm", start)]
        assert "v_accvgpr" not in body and "scratch_" not in body and "buffer_store" not in body, name
        waits = [int(w) for w in re.findall(r"s_waitcnt vmcnt\((\d+)\)", body)]
        step = 7 + 2  # seven coefficient pairs, the right-hand side, the store into the outflow record
        block = 4 + 4 * step + 4  # + four polls, two flushes of two stores
        want = sorted([block - step] * 2 + [block - step - 2] * 2 + [block - 4])
        assert sorted(w for w in waits if w > 0) == want, (name, waits, want)
        # (drains: the ticket, the pencil table, the queue's first fill, the re-poll loop, the end of a pencil, the debug stores)
        assert sum(1 for w in waits if w == 0) <= 8, (name, waits)
        wide = [m.end() for m in re.finditer(r"global_store_dwordx4[^\n]*\n", body)]
        assert wide or "IfLb" in name, name  # (fp32 pairs are 8-byte stores)
        for e in wide:
            assert body[e:e + 40].lstrip().startswith("s_nop 1"), (name, body[e:e + 60])


# ------------------------------------------------------------------ the plane-ahead loads of the red-black SGS kernel
def test_red_black_sgs_kernel_keeps_its_loads_in_flight_across_the_barriers(tmp_path):
    """k_mc_rb (csrc/mcsgs.hip) issues the global loads of a stage one plane ahead and relies on the COMPILER counting its waits:
    every lane issues every load (clamped addresses), so the loads in flight are a constant.  A load under a divergent branch,
    a __syncthreads() or a spill would turn the counted waits of the plane loop into drains again (3.0 -> 3.4 ms at 512^3).
    Checked on the ISA of both precisions: no scratch, no spills, and inside the plane loop -- the last loop with four
    barriers -- every wait in front of the stages leaves loads in flight."""
    import re
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "mc.s"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rocalution_amd", "csrc"),
           "--cuda-device-only", "-S", os.path.join(ROOT, "rocalution_amd", "csrc", "mcsgs.hip"), "-o", str(out)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:]
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels:"):]
    kern = re.findall(r"\.name:\s+(\S*k_mc_rb\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\s+\.vgpr_spill_count:\s+(\d+)",
                      meta, flags=re.S)
    assert len(kern) == 2, [k[0] for k in kern]
    for name, scratch, vgpr, spill in kern:
        assert int(scratch) == 0 and int(spill) == 0 and int(vgpr) <= 256, (name, scratch, vgpr, spill)
        start = text.index("\n" + name + ":")
        lines = [l.strip() for l in text[start:text.index("s_endpgm", start)].split("\n")]
        assert not any(l.startswith("scratch_") for l in lines), name
        labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
        # the plane loop: the widest backward branch
        back = [(labels[m.group(1)], i) for i, l in enumerate(lines)
                for m in [re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", l)] if m and labels.get(m.group(1), 1 << 30) < i]
        lo, hi = max(back, key=lambda b: b[1] - b[0])
        loop = lines[lo:hi]
        assert sum(1 for l in loop if l == "s_barrier") == 4, (name, sum(1 for l in loop if l == "s_barrier"))
        loads = sum(1 for l in loop if l.startswith("global_load"))
        assert loads >= 30, (name, loads)  # rhs, 1/d and two stages of eight arrays, for every cell a thread has
        waits = [int(w) for l in loop for w in re.findall(r"vmcnt\((\d+)\)", l)]
        assert waits and min(waits) >= 8, (name, waits)


# ------------------------------------------------------------------ the wave-private row walk and its three kernels
def test_wave_row_walk_kernels_have_no_scratch_and_no_spills(tmp_path):
    """k_csr_wr (csrc/spmv.hip), k_csr_wide (csrc/spmv_wide.hip) and k_tns_tri (csrc/tns.hip) are callers of one staging and one
    walk (csrc/wave_rows.hpp), whose registers hold the packets of a pass and GW gathers per row: every instantiation, compiled
    for gfx950 with the library's flags, without scratch, without spills and within 256 VGPRs.  From the kernel metadata alone."""
    import concurrent.futures as cf
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")

    def metadata(unit):
        out = tmp_path / (unit + ".s")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rocalution_amd", "csrc"),
               "--cuda-device-only", "-S", os.path.join(ROOT, "rocalution_amd", "csrc", unit + ".hip"), "-o", str(out)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        assert p.returncode == 0, p.stdout[-2000:]
        text = out.read_text()
        return text[text.index("amdhsa.kernels:"):]

    # {fp64, fp32} x: k_csr_wr {MODE 0, 0 + DOT, 1, 2} x {PAT} x {GW 8, 14, 28}; k_csr_wide the same at one GW; k_tns_tri
    # {lower, upper} x {STAGE 0, 1}
    want = {"spmv": ("k_csr_wr", 48), "spmv_wide": ("k_csr_wide", 16), "tns": ("k_tns_tri", 8)}
    with cf.ThreadPoolExecutor(3) as ex:
        metas = dict(zip(want, ex.map(metadata, want)))
    for unit, (kname, count) in want.items():
        kern = re.findall(r"\.name:\s+(\S*" + kname + r"\S*).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)\s+"
                          r"\.vgpr_spill_count:\s+(\d+)", metas[unit], flags=re.S)
        assert len(kern) == count, (unit, [k[0] for k in kern])
        for name, scratch, vgpr, spill in kern:
            assert int(scratch) == 0 and int(spill) == 0 and int(vgpr) <= 256, (name, scratch, vgpr, spill)


# ------------------------------------------------------------------ the reference's own 3-D operator (host restatement)
def test_laplace27_host_generator_is_the_reference_loop():
    from rocalution_amd import generators as gen
    import numpy as np
    """generators.laplace27 against a literal walk of the reference's three nested offset loops (utility.hpp:134-170)"""
    nx, ny, nz = 4, 3, 5
    rp, ci, va = gen.laplace27(nx, ny, nz)
    cols, vals, ptr = [], [], [0]
    for iz in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                row = iz * ny * nx + iy * nx + ix
                for sz in (-1, 0, 1):
                    if not (-1 < iz + sz < nz):
                        continue
                    for sy in (-1, 0, 1):
                        if not (-1 < iy + sy < ny):
                            continue
                        for sx in (-1, 0, 1):
                            if -1 < ix + sx < nx:
                                col = row + sz * ny * nx + sy * nx + sx
                                cols.append(col); vals.append(26.0 if col == row else -1.0)
                ptr.append(len(cols))
    assert np.array_equal(rp, ptr) and np.array_equal(ci, cols) and np.array_equal(va, vals)
    rp, ci, va = gen.laplace27(6)
    assert len(rp) - 1 == 216 and np.diff(rp).max() == 27 and np.diff(rp).min() == 8
