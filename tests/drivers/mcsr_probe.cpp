// tests/drivers/mcsr_probe.cpp -- TEST INFRASTRUCTURE.  Records what the genuine rocALUTION library computes for the MCSR
// format, for tools/gen_golden_mcsr.py.  It includes nothing but the installed public header, links the installed library,
// disables the accelerator and runs on one OpenMP thread.
//   mcsr_probe <indir> <outdir> [solve]
//       indir: hdr.bin (int64 n, nnz), rowptr.bin / col.bin (int32), val.bin, x.bin, y.bin, rhs.bin (double)
// Per matrix, in fp64 (no suffix) and fp32 (_f32; the inputs cast): format (the format after ConvertToMCSR(), int32: 2, or 1
// where the library refuses), and where it converts: spmv_mcsr = A x, spmv_mcsr_add = y - 0.75 A x (ApplyAdd), back_rowptr /
// _col / _val (a clone converted back to CSR) and mcsr_rowptr / _col / _val (LeaveDataPtrMCSR).  With `solve`, fp64 only:
// cg_jacobi_mcsr_{meta,hist,x} of CG + Jacobi with the library's default tolerances on the MCSR operator (converted before
// Build()), right-hand side rhs.bin, zero initial guess.
#include <rocalution/rocalution.hpp>

#include <cstdint>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace rocalution;

static std::string g_out;

template <typename X>
static void dump(const std::string& name, const X* p, size_t n)
{
    std::ofstream f(g_out + "/" + name + ".bin", std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), sizeof(X) * n);
}
template <typename X>
static std::vector<X> slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if(!f)
    {
        std::cerr << "cannot open " << path << std::endl;
        exit(2);
    }
    size_t         sz = f.tellg();
    std::vector<X> v(sz / sizeof(X));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), sz);
    return v;
}
template <typename T>
static void dump_vec(const std::string& name, const LocalVector<T>& v)
{
    std::vector<T> h(v.GetSize());
    if(!h.empty())
        v.CopyToHostData(h.data());
    dump(name, h.data(), h.size());
}
template <typename T>
static void load_vec(LocalVector<T>& v, const std::vector<double>& d)
{
    std::vector<T> h(d.begin(), d.end());
    v.Allocate("v", (int64_t)h.size());
    if(!h.empty())
        v.CopyFromHostData(h.data());
}

template <typename T>
static void run(const std::string& in, int64_t n, int64_t nnz, const std::string& sfx, bool solve)
{
    std::vector<int32_t> rp = slurp<int32_t>(in + "/rowptr.bin"), ci = slurp<int32_t>(in + "/col.bin");
    std::vector<double>  vd = slurp<double>(in + "/val.bin");
    std::vector<T>       va(vd.begin(), vd.end());
    LocalMatrix<T>       mat;
    mat.AllocateCSR("A", nnz, n, n);
    mat.CopyFromCSR(rp.data(), ci.data(), va.data());
    mat.ConvertToMCSR();
    int32_t fmt = (int32_t)mat.GetFormat();
    dump("format" + sfx, &fmt, 1);
    if(mat.GetFormat() != MCSR)
        return;
    LocalVector<T> x, y;
    load_vec(x, slurp<double>(in + "/x.bin"));
    y.Allocate("y", n);
    mat.Apply(x, &y);
    dump_vec("spmv_mcsr" + sfx, y);
    load_vec(y, slurp<double>(in + "/y.bin"));
    mat.ApplyAdd(x, static_cast<T>(-0.75), &y);
    dump_vec("spmv_mcsr_add" + sfx, y);
    {
        LocalMatrix<T> back;
        back.CloneFrom(mat);
        back.ConvertToCSR();
        std::vector<int32_t> brp(back.GetM() + 1), bci(back.GetNnz());
        std::vector<T>       bva(back.GetNnz());
        back.CopyToCSR(brp.data(), bci.data(), bva.data());
        dump("back_rowptr" + sfx, brp.data(), brp.size());
        dump("back_col" + sfx, bci.data(), bci.size());
        dump("back_val" + sfx, bva.data(), bva.size());
    }
    if(solve)
    {
        LocalVector<T> rhs, sol;
        load_vec(rhs, slurp<double>(in + "/rhs.bin"));
        sol.Allocate("x", n);
        sol.Zeros();
        CG<LocalMatrix<T>, LocalVector<T>, T>     ls;
        Jacobi<LocalMatrix<T>, LocalVector<T>, T> p;
        ls.SetOperator(mat);
        ls.SetPreconditioner(p);
        ls.Build();
        ls.Verbose(0);
        ls.RecordResidualHistory();
        ls.Solve(rhs, &sol);
        int32_t fmt_after = (int32_t)mat.GetFormat();
        dump("format_after_solve" + sfx, &fmt_after, 1);
        ls.RecordHistory(g_out + "/cg_jacobi_mcsr_hist.txt");
        double meta[3] = {(double)ls.GetIterationCount(), (double)ls.GetSolverStatus(), (double)ls.GetCurrentResidual()};
        dump("cg_jacobi_mcsr_meta", meta, 3);
        dump_vec("cg_jacobi_mcsr_x", sol);
        ls.Clear();
    }
    int *mro = NULL, *mci = NULL;
    T*   mva = NULL;
    mat.LeaveDataPtrMCSR(&mro, &mci, &mva);
    dump("mcsr_rowptr" + sfx, mro, (size_t)n + 1);
    dump("mcsr_col" + sfx, mci, (size_t)nnz);
    dump("mcsr_val" + sfx, mva, (size_t)nnz);
    free_host(&mro);
    free_host(&mci);
    free_host(&mva);
}

int main(int argc, char* argv[])
{
    if(argc < 3)
    {
        std::cerr << argv[0] << " <indir> <outdir> [solve]" << std::endl;
        return 1;
    }
    const std::string in = argv[1];
    g_out                = argv[2];
    const bool solve     = argc > 3 && std::string(argv[3]) == "solve";
    disable_accelerator_rocalution(true);
    init_rocalution();
    set_omp_threads_rocalution(1);
    std::vector<int64_t> hdr = slurp<int64_t>(in + "/hdr.bin");
    run<double>(in, hdr[0], hdr[1], "", solve);
    run<float>(in, hdr[0], hdr[1], "_f32", false);
    stop_rocalution();
    return 0;
}
