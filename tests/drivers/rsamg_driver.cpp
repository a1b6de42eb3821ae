// tests/drivers/rsamg_driver.cpp -- Ruge-Stueben AMG written against include/rocalution the way the reference's sample
// does it (the call sequence of clients/samples/rs-amg.cpp): the AMG as a solver, or CG preconditioned by it, on a matrix
// file or the built-in Laplacian.
// Usage: rsamg_driver <matrix.mtx | poisson:N> <amg|cg|vcycle> [greedy|pmis] [direct|extpi] [ff1] [coarsest rows]
//   without the optional arguments the class's defaults hold (Greedy, Direct, FF1 off); the coarsest level is 20 rows
//   unless given.  Prints LEVEL lines (rows, entries per level), the residual history (HIST lines) and one RESULT line,
//   which tests/test_gpu_rsamg.py compares with the genuine library's run of the same setup (tests/drivers/rsamg_probe.cpp).
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include <rocalution/rocalution.hpp>

using namespace rocalution;

int main(int argc, char* argv[])
{
    if(argc < 3)
    {
        std::cerr << argv[0] << " <matrix.mtx | poisson:N> <amg|cg|vcycle> [greedy|pmis] [direct|extpi] [ff1] [coarsest]" << std::endl;
        return 1;
    }
    init_rocalution();
    LocalMatrix<double> mat;
    LocalVector<double> x, rhs, e;
    const std::string   src = argv[1], mode = argv[2];
    if(src.compare(0, 8, "poisson:") == 0)
    {
        mat.MoveToAccelerator();
        mat.GeneratePoisson7(atoi(src.c_str() + 8)); // extension: 3-D 7-point operator built on the device
    }
    else
    {
        mat.ReadFileMTX(src);
        mat.MoveToAccelerator();
    }
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    rhs.Allocate("rhs", mat.GetM());
    e.Allocate("e", mat.GetN());
    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();

    RugeStuebenAMG<LocalMatrix<double>, LocalVector<double>, double> amg;
    CG<LocalMatrix<double>, LocalVector<double>, double>             cg;
    int                                                              coarsest = 20;
    for(int a = 3; a < argc; ++a)
    {
        const std::string o = argv[a];
        if(o == "pmis")
            amg.SetCoarseningStrategy(PMIS);
        else if(o == "greedy")
            amg.SetCoarseningStrategy(Greedy);
        else if(o == "extpi")
            amg.SetInterpolationType(ExtPI);
        else if(o == "direct")
            amg.SetInterpolationType(Direct);
        else if(o == "ff1")
            amg.SetInterpolationFF1Limit(true);
        else
            coarsest = atoi(o.c_str());
    }
    amg.SetOperator(mat);
    amg.SetCoarsestLevel(coarsest);
    amg.Verbose(0);
    IterativeLinearSolver<LocalMatrix<double>, LocalVector<double>, double>* ls = &amg;
    if(mode == "amg")
        amg.InitMaxIter(60);
    else if(mode == "vcycle") // one V-cycle of the class from x = 0: what a Krylov solver gets from it as a preconditioner
        amg.InitMaxIter(1);
    else
    {
        cg.SetOperator(mat);
        cg.SetPreconditioner(amg);
        cg.InitMaxIter(100);
        ls = &cg;
    }
    ls->Verbose(0);
    ls->RecordResidualHistory();
    double t0 = rocalution_time();
    ls->Build();
    _rocalution_sync();
    double t1 = rocalution_time();
    amg.Print();
    const int levels = amg.GetNumLevels();
    for(int l = 0; l < levels; ++l)
    {
        int64_t rows = 0, nnz = 0;
        amg.GetLevelSize(l, &rows, &nnz);
        std::cout << "LEVEL " << l << " rows=" << rows << " nnz=" << nnz << std::endl;
    }
    ls->Solve(rhs, &x);
    _rocalution_sync();
    double t2 = rocalution_time();
    std::cout << "TIMING build_s=" << (t1 - t0) / 1e6 << " solve_s=" << (t2 - t1) / 1e6 << std::endl;
    std::cout.precision(17);
    const std::vector<double> h = ls->GetResidualHistory();
    for(size_t i = 0; i < h.size(); ++i)
        std::cout << "HIST " << h[i] << std::endl;
    std::vector<double> hx((size_t)x.GetSize());
    x.CopyToHostData(hx.data());
    for(size_t i = 0; i < hx.size(); ++i)
        std::cout << "X " << hx[i] << std::endl;
    e.ScaleAdd(-1.0, x);
    std::cout << "RESULT mode=" << mode << " levels=" << levels << " iters=" << ls->GetIterationCount()
              << " status=" << ls->GetSolverStatus() << " residual=" << ls->GetCurrentResidual() << " error=" << e.Norm()
              << std::endl;
    ls->Clear();
    stop_rocalution();
    return 0;
}
