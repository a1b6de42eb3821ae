// tests/drivers/multielim_probe.cpp -- TEST INFRASTRUCTURE.  Records what the genuine rocALUTION library computes for the
// MultiElimination preconditioner, for tools/gen_golden_multielim.py.  It includes nothing but the installed public header,
// links the installed library, disables the accelerator and runs on one OpenMP thread.
//   multielim_probe <indir> <outdir>
//     indir: hdr.bin (int64 n, nnz, krylov: 1 = also the CG run), rowptr.bin / col.bin (int32), val.bin, rhs.bin (double)
// In fp64 and fp32 (suffix _f32): size and perm of MaximalIndependentSet; AA of one elimination for drop_off 0 (aa0_*) and
// for a positive drop_off (aad_*); Compress(drop) of the operator itself (cmp_*); for levels 1 and 2 with Jacobi as the
// last block and drop_off 0: the sizes of the diagonal blocks (me<level>_sizes) and Solve(rhs) (me<level>_x).
// The positive drop_off (drop.bin) is derived from the fp64 AA: half way between the smallest and the largest magnitude of
// its off-diagonal entries, or 1.5 times that magnitude when they are all alike (then every off-diagonal entry goes).
// krylov, fp64: CG + MultiElimination(MultiColoredILU(0), 2, drop) on rhs = A 1 -- iterations, status, residual, history, x.
#include <rocalution/rocalution.hpp>

#include <algorithm>
#include <cmath>
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
static void get_csr(const LocalMatrix<T>& m, std::vector<int32_t>& rp, std::vector<int32_t>& ci, std::vector<T>& va)
{
    rp.assign(m.GetM() + 1, 0);
    ci.resize(m.GetNnz());
    va.resize(m.GetNnz());
    if(m.GetNnz() > 0)
        m.CopyToCSR(rp.data(), ci.data(), va.data());
}
template <typename T>
static void dump_csr(const std::string& name, const LocalMatrix<T>& m)
{
    std::vector<int32_t> rp, ci;
    std::vector<T>       va;
    get_csr(m, rp, ci, va);
    int64_t shape[3] = {(int64_t)m.GetM(), (int64_t)m.GetN(), (int64_t)m.GetNnz()};
    dump(name + "_shape", shape, 3);
    dump(name + "_rowptr", rp.data(), rp.size());
    dump(name + "_col", ci.data(), ci.size());
    dump(name + "_val", va.data(), va.size());
}

// the blocks are protected members of the public class: a derived class may read them
template <typename T>
struct OpenME : public MultiElimination<LocalMatrix<T>, LocalVector<T>, T>
{
    const LocalMatrix<T>& AA(void) const
    {
        return this->AA_;
    }
    std::vector<int64_t> sizes(void) const
    {
        std::vector<int64_t> s;
        s.push_back(this->GetSizeDiagBlock());
        if(this->AA_me_ != NULL)
            s.push_back(this->AA_me_->GetSizeDiagBlock());
        return s;
    }
};

template <typename T>
static void run(const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, const std::vector<double>& vd,
                const std::vector<double>& rd, int64_t n, int64_t nnz, const std::string& sfx, double* drop)
{
    std::vector<T> va(vd.begin(), vd.end()), hr(rd.begin(), rd.end());
    LocalMatrix<T> mat;
    mat.AllocateCSR("A", nnz, n, n);
    mat.CopyFromCSR(rp.data(), ci.data(), va.data());
    {
        LocalVector<int> perm;
        int              size = 0;
        mat.MaximalIndependentSet(size, &perm);
        std::vector<int32_t> hp(perm.GetSize());
        perm.CopyToHostData(hp.data());
        int64_t s64 = size;
        dump("size" + sfx, &s64, 1);
        dump("perm" + sfx, hp.data(), hp.size());
    }
    for(int pass = 0; pass < 2; ++pass)
    {
        Jacobi<LocalMatrix<T>, LocalVector<T>, T> jac;
        OpenME<T>                                 me;
        me.SetOperator(mat);
        me.Set(jac, 1, pass ? *drop : 0.0);
        me.Build();
        dump_csr(std::string(pass ? "aad" : "aa0") + sfx, me.AA());
        if(pass == 0 && *drop < 0.0)
        {
            std::vector<int32_t> arp, aci;
            std::vector<T>       ava;
            get_csr(me.AA(), arp, aci, ava);
            double lo = 0.0, hi = 0.0;
            bool   any = false;
            for(int64_t i = 0; i + 1 < (int64_t)arp.size(); ++i)
                for(int32_t j = arp[i]; j < arp[i + 1]; ++j)
                    if(aci[j] != i)
                    {
                        const double a = std::abs((double)ava[j]);
                        lo             = any ? std::min(lo, a) : a;
                        hi             = any ? std::max(hi, a) : a;
                        any            = true;
                    }
            *drop = (hi > lo) ? 0.5 * (lo + hi) : 1.5 * hi;
        }
        me.Clear();
    }
    {
        LocalMatrix<T> cmp;
        cmp.CloneFrom(mat);
        cmp.Compress(*drop);
        dump_csr("cmp" + sfx, cmp);
    }
    LocalVector<T> rhs, x;
    rhs.Allocate("rhs", n);
    x.Allocate("x", n);
    rhs.CopyFromData(hr.data());
    for(int level = 1; level <= 2; ++level)
    {
        Jacobi<LocalMatrix<T>, LocalVector<T>, T> jac;
        OpenME<T>                                 me;
        me.SetOperator(mat);
        me.Set(jac, level, 0.0);
        me.Build();
        std::vector<int64_t> sz = me.sizes();
        const std::string    tag = "me" + std::to_string(level);
        dump(tag + "_sizes" + sfx, sz.data(), sz.size());
        x.Zeros();
        me.Solve(rhs, &x);
        std::vector<T> hx((size_t)n);
        x.CopyToHostData(hx.data());
        dump(tag + "_x" + sfx, hx.data(), hx.size());
        me.Clear();
    }
}

int main(int argc, char* argv[])
{
    if(argc < 3)
    {
        std::cerr << argv[0] << " <indir> <outdir>" << std::endl;
        return 1;
    }
    const std::string in = argv[1];
    g_out                = argv[2];
    disable_accelerator_rocalution(true);
    init_rocalution();
    set_omp_threads_rocalution(1);
    std::vector<int64_t> hdr = slurp<int64_t>(in + "/hdr.bin");
    const int64_t        n = hdr[0], nnz = hdr[1];
    std::vector<int32_t> rp = slurp<int32_t>(in + "/rowptr.bin"), ci = slurp<int32_t>(in + "/col.bin");
    std::vector<double>  va = slurp<double>(in + "/val.bin"), rd = slurp<double>(in + "/rhs.bin");
    double               drop = -1.0;
    run<double>(rp, ci, va, rd, n, nnz, "", &drop);
    run<float>(rp, ci, va, rd, n, nnz, "_f32", &drop);
    dump("drop", &drop, 1);
    if(hdr[2] != 0)
    {
        LocalMatrix<double> mat;
        mat.AllocateCSR("A", nnz, n, n);
        mat.CopyFromCSR(rp.data(), ci.data(), va.data());
        LocalVector<double> ones, rhs, x;
        ones.Allocate("ones", n);
        rhs.Allocate("rhs", n);
        x.Allocate("x", n);
        ones.Ones();
        mat.Apply(ones, &rhs);
        x.Zeros();
        CG<LocalMatrix<double>, LocalVector<double>, double>               cg;
        MultiElimination<LocalMatrix<double>, LocalVector<double>, double> p;
        MultiColoredILU<LocalMatrix<double>, LocalVector<double>, double>  mcilu;
        mcilu.Set(0);
        p.Set(mcilu, 2, drop);
        cg.SetOperator(mat);
        cg.SetPreconditioner(p);
        cg.Verbose(0);
        cg.Build();
        cg.RecordResidualHistory();
        cg.Solve(rhs, &x);
        const std::string hf = g_out + "/cg_me_hist.txt";
        if(cg.GetIterationCount() > 0)
            cg.RecordHistory(hf);
        else
        {
            std::ofstream empty(hf.c_str());
        }
        double meta[3] = {(double)cg.GetIterationCount(), (double)cg.GetSolverStatus(), cg.GetCurrentResidual()};
        dump("cg_me_meta", meta, 3);
        std::vector<double> hx((size_t)n);
        x.CopyToHostData(hx.data());
        dump("cg_me_x", hx.data(), hx.size());
        cg.Clear();
    }
    stop_rocalution();
    return 0;
}
