// tests/drivers/rsamg_probe.cpp -- TEST INFRASTRUCTURE.  Records what the genuine rocALUTION library computes for
// Ruge-Stueben AMG, for tools/gen_golden_rsamg.py.  It includes nothing but the installed public header, links the
// installed library, disables the accelerator and runs on one OpenMP thread (deterministic sums).
//   rsamg_probe <indir> <outdir>      indir: hdr.bin (int64 n, nnz), rowptr.bin / col.bin (int32), val.bin (double)
// Per matrix, in fp64 and fp32: the Greedy and PMIS C/F maps and S; the Direct P and the extended+i P (FF1 off / on) from
// both maps; the first coarse operator of the ExtPI P (FF1 off) of both maps.  In fp64: {Greedy, PMIS} x {Direct, ExtPI} x
// {solver, CG preconditioner} runs with the coarsest level at 20 rows -- levels, rows / nnz per level, iterations, status,
// residual, history file, x.
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
static void dump_csr(const std::string& name, const LocalMatrix<T>& m)
{
    std::vector<int32_t> rp(m.GetM() + 1, 0), ci(m.GetNnz());
    std::vector<T>       va(m.GetNnz());
    if(m.GetNnz() > 0)
        m.CopyToCSR(rp.data(), ci.data(), va.data());
    int64_t shape[3] = {(int64_t)m.GetM(), (int64_t)m.GetN(), (int64_t)m.GetNnz()};
    dump(name + "_shape", shape, 3);
    dump(name + "_rowptr", rp.data(), rp.size());
    dump(name + "_col", ci.data(), ci.size());
    dump(name + "_val", va.data(), va.size());
}
static void dump_map(const std::string& name, const LocalVector<int>& cf, const LocalVector<bool>& S)
{
    std::vector<int32_t> hcf(cf.GetSize()), hs(S.GetSize());
    if(!hcf.empty())
        cf.CopyToHostData(hcf.data());
    bool* tb = new bool[S.GetSize() + 1];
    if(S.GetSize() > 0)
        S.CopyToHostData(tb);
    for(size_t k = 0; k < hs.size(); ++k)
        hs[k] = tb[k] ? 1 : 0;
    delete[] tb;
    dump(name + "_cf", hcf.data(), hcf.size());
    dump(name + "_S", hs.data(), hs.size());
}

// the hierarchy's operators are protected members of the public class: a derived class may read their sizes
template <typename T>
struct SizedRS : public RugeStuebenAMG<LocalMatrix<T>, LocalVector<T>, T>
{
    std::vector<double> sizes()
    {
        std::vector<double> s;
        s.push_back((double)this->op_->GetM());
        s.push_back((double)this->op_->GetNnz());
        for(int l = 0; l + 1 < this->levels_; ++l)
        {
            s.push_back((double)this->op_level_[l]->GetM());
            s.push_back((double)this->op_level_[l]->GetNnz());
        }
        return s;
    }
};

template <typename T>
static void primitives(const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, const std::vector<double>& vd,
                       int64_t n, int64_t nnz, const std::string& sfx)
{
    std::vector<T> va(vd.begin(), vd.end());
    LocalMatrix<T> mat;
    mat.AllocateCSR("A", nnz, n, n);
    mat.CopyFromCSR(rp.data(), ci.data(), va.data());
    for(int strat = 0; strat < 2; ++strat)
    {
        const std::string tag = (strat ? std::string("pmis") : std::string("greedy")) + sfx;
        LocalVector<int>  cf;
        LocalVector<bool> S;
        if(strat)
            mat.RSPMISCoarsening(0.25f, &cf, &S);
        else
            mat.RSCoarsening(0.25f, &cf, &S);
        dump_map(tag, cf, S);
        LocalMatrix<T> P;
        mat.RSDirectInterpolation(cf, S, &P);
        dump_csr("direct_" + tag, P);
        for(int ff1 = 0; ff1 < 2; ++ff1)
        {
            LocalMatrix<T> E;
            mat.RSExtPIInterpolation(cf, S, ff1 != 0, &E);
            dump_csr(std::string("extpi_") + tag + (ff1 ? "_ff1" : "_ff0"), E);
            if(!ff1 && E.GetN() > 0)
            {
                LocalMatrix<T> R, Ac;
                E.Transpose(&R);
                Ac.TripleMatrixProduct(R, mat, E);
                dump_csr("Ac_" + tag, Ac);
            }
        }
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
    std::vector<double>  va = slurp<double>(in + "/val.bin");
    primitives<double>(rp, ci, va, n, nnz, "");
    primitives<float>(rp, ci, va, n, nnz, "_f32");
    if(hdr.size() > 2 && hdr[2] == 0) // primitives only
    {
        stop_rocalution();
        return 0;
    }
    LocalMatrix<double> mat;
    mat.AllocateCSR("A", nnz, n, n);
    mat.CopyFromCSR(rp.data(), ci.data(), va.data());
    LocalVector<double> ones, rhs, x;
    ones.Allocate("ones", n);
    rhs.Allocate("rhs", n);
    x.Allocate("x", n);
    ones.Ones();
    mat.Apply(ones, &rhs);
    for(int strat = 0; strat < 2; ++strat)
        for(int interp = 0; interp < 2; ++interp)
            for(int mode = 0; mode < 2; ++mode)
            {
                const std::string tag = std::string(mode ? "cg_" : "amg_") + (strat ? "pmis_" : "greedy_")
                                        + (interp ? "extpi" : "direct");
                SizedRS<double>& amg = *new SizedRS<double>;
                amg.SetOperator(mat);
                amg.SetCoarseningStrategy(strat ? PMIS : Greedy);
                amg.SetInterpolationType(interp ? ExtPI : Direct);
                amg.SetCoarsestLevel(20);
                amg.Verbose(0);
                CG<LocalMatrix<double>, LocalVector<double>, double>                     cg;
                IterativeLinearSolver<LocalMatrix<double>, LocalVector<double>, double>* ls = &amg;
                if(mode == 0)
                    amg.InitMaxIter(60);
                else
                {
                    cg.SetOperator(mat);
                    cg.SetPreconditioner(amg);
                    cg.InitMaxIter(100);
                    ls = &cg;
                }
                ls->Verbose(0);
                ls->Build();
                std::vector<double> sz = amg.sizes();
                dump(tag + "_sizes", sz.data(), sz.size());
                x.Zeros();
                ls->RecordResidualHistory();
                ls->Solve(rhs, &x);
                const std::string hf = g_out + "/" + tag + "_hist.txt";
                if(ls->GetIterationCount() > 0)
                    ls->RecordHistory(hf);
                else
                {
                    std::ofstream empty(hf.c_str());
                }
                double meta[4] = {(double)ls->GetIterationCount(), (double)ls->GetSolverStatus(), ls->GetCurrentResidual(),
                                  (double)amg.GetNumLevels()};
                dump(tag + "_meta", meta, 4);
                std::vector<double> hx((size_t)n);
                x.CopyToHostData(hx.data());
                dump(tag + "_x", hx.data(), hx.size());
                ls->Clear();
            }
    stop_rocalution();
    return 0;
}
