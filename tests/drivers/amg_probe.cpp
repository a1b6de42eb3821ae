// tests/drivers/amg_probe.cpp -- TEST INFRASTRUCTURE.  Records what the genuine rocALUTION library computes for the
// aggregation-AMG setup, for tools/gen_golden_amg.py.  It includes nothing but the installed public header, links the
// installed library, disables the accelerator and runs on one OpenMP thread.
//   amg_probe <indir> <outdir>      indir: hdr.bin (int64 n, nnz), rowptr.bin / col.bin (int32), val.bin (double)
// Per matrix, in fp64 (no suffix) and fp32 (_f32), with eps = 0.01: for the Greedy and the PMIS aggregation the
// connections, aggregates and root nodes (as int32), the unsmoothed prolongator and the smoothed prolongators for
// (relax 2/3, lumping 0) and (relax 0.5, lumping 1).
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
static void dump_i64(const std::string& name, const LocalVector<int64_t>& v)
{
    std::vector<int64_t> h(v.GetSize());
    if(!h.empty())
        v.CopyToHostData(h.data());
    std::vector<int32_t> o(h.begin(), h.end());
    dump(name, o.data(), o.size());
}
static void dump_bool(const std::string& name, const LocalVector<bool>& v)
{
    std::vector<int32_t> o(v.GetSize());
    bool*                tb = new bool[v.GetSize() + 1];
    if(v.GetSize() > 0)
        v.CopyToHostData(tb);
    for(size_t k = 0; k < o.size(); ++k)
        o[k] = tb[k] ? 1 : 0;
    delete[] tb;
    dump(name, o.data(), o.size());
}

template <typename T>
static void setup(const std::vector<int32_t>& rp, const std::vector<int32_t>& ci, const std::vector<double>& vd, int64_t n,
                  int64_t nnz, const std::string& sfx)
{
    std::vector<T> va(vd.begin(), vd.end());
    LocalMatrix<T> mat;
    mat.AllocateCSR("A", nnz, n, n);
    mat.CopyFromCSR(rp.data(), ci.data(), va.data());
    for(int strat = 0; strat < 2; ++strat)
    {
        const std::string    tag = (strat ? std::string("pmis") : std::string("greedy")) + sfx;
        LocalVector<bool>    conn;
        LocalVector<int64_t> agg, roots;
        if(strat)
            mat.AMGPMISAggregate(static_cast<T>(0.01), &conn, &agg, &roots);
        else
            mat.AMGGreedyAggregate(static_cast<T>(0.01), &conn, &agg, &roots);
        dump_bool(tag + "_conn", conn);
        dump_i64(tag + "_agg", agg);
        dump_i64(tag + "_roots", roots);
        LocalMatrix<T> P;
        mat.AMGUnsmoothedAggregation(agg, roots, &P);
        dump_csr("ua_" + tag, P);
        LocalMatrix<T> S0, S1;
        mat.AMGSmoothedAggregation(static_cast<T>(2.0 / 3.0), conn, agg, roots, &S0, 0);
        dump_csr("sa0_" + tag, S0);
        mat.AMGSmoothedAggregation(static_cast<T>(0.5), conn, agg, roots, &S1, 1);
        dump_csr("sa1_" + tag, S1);
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
    setup<double>(rp, ci, va, n, nnz, "");
    setup<float>(rp, ci, va, n, nnz, "_f32");
    stop_rocalution();
    return 0;
}
