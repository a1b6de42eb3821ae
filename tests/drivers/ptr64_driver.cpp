// ptr64_driver -- the C++ layer in its 64-bit PtrType flavour (-DRAMD_PTR64, the reference's BUILD_PTRTYPE_64): a user's
// int64_t row offsets go in through SetDataPtrCSR, come back through CopyToCSR, and CG + Jacobi on the 32^3 Poisson operator
// runs as it does from int32 offsets.  "ptr64_driver check" stops after the host-side checks (no accelerator needed).
//   g++ -std=c++14 -DRAMD_PTR64 -Iinclude tests/drivers/ptr64_driver.cpp -Lrocalution_amd -lrocalution_amd
#include <rocalution/rocalution.hpp>

#include <cstring>
#include <iostream>
#include <vector>

using namespace rocalution;

static_assert(sizeof(rocalution::PtrType) == 8, "-DRAMD_PTR64 makes PtrType a 64-bit integer");

// the 3-D 7-point operator, rows x fastest, ascending columns
static void poisson7(int N, std::vector<PtrType>& rp, std::vector<int>& ci, std::vector<double>& va)
{
    rp.assign(1, 0);
    for(int z = 0; z < N; ++z)
        for(int y = 0; y < N; ++y)
            for(int x = 0; x < N; ++x)
            {
                const int  r     = (z * N + y) * N + x;
                const int  nb[7] = {r - N * N, r - N, r - 1, r, r + 1, r + N, r + N * N};
                const bool ok[7] = {z > 0, y > 0, x > 0, true, x < N - 1, y < N - 1, z < N - 1};
                for(int k = 0; k < 7; ++k)
                    if(ok[k])
                    {
                        ci.push_back(nb[k]);
                        va.push_back(k == 3 ? 6.0 : -1.0);
                    }
                rp.push_back((PtrType)ci.size());
            }
}

int main(int argc, char* argv[])
{
    const int            N = 32;
    std::vector<PtrType> rp;
    std::vector<int>     ci;
    std::vector<double>  va;
    poisson7(N, rp, ci, va);
    const int     n   = N * N * N;
    const int64_t nnz = (int64_t)ci.size();
    if(argc > 1 && strcmp(argv[1], "check") == 0)
    {
        // host side only: the arrays pass through the object unchanged
        LocalMatrix<double> h;
        h.AllocateCSR("h", nnz, n, n);
        h.CopyFromCSR(rp.data(), ci.data(), va.data());
        std::vector<PtrType> rp2(rp.size());
        std::vector<int>     ci2(ci.size());
        std::vector<double>  va2(va.size());
        h.CopyToCSR(rp2.data(), ci2.data(), va2.data());
        if(rp2 != rp || ci2 != ci || va2 != va)
        {
            std::cout << "ptr64_driver: host round trip differs" << std::endl;
            return 1;
        }
        std::cout << "ptr64_driver check ok" << std::endl;
        return 0;
    }
    init_rocalution();
    LocalMatrix<double> mat;
    LocalVector<double> x, rhs, e;
    {
        PtrType* p_rp = new PtrType[rp.size()];
        int*     p_ci = new int[ci.size()];
        double*  p_va = new double[va.size()];
        std::copy(rp.begin(), rp.end(), p_rp);
        std::copy(ci.begin(), ci.end(), p_ci);
        std::copy(va.begin(), va.end(), p_va);
        mat.SetDataPtrCSR(&p_rp, &p_ci, &p_va, "poisson32", nnz, n, n);
    }
    mat.MoveToAccelerator();
    // the device object gives the same arrays back as int64_t offsets
    {
        std::vector<PtrType> rp2(rp.size());
        std::vector<int>     ci2(ci.size());
        std::vector<double>  va2(va.size());
        mat.CopyToCSR(rp2.data(), ci2.data(), va2.data());
        if(rp2 != rp || ci2 != ci || va2 != va)
        {
            std::cout << "ptr64_driver: device round trip differs" << std::endl;
            return 1;
        }
    }
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", n);
    rhs.Allocate("rhs", n);
    e.Allocate("e", n);
    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();
    CG<LocalMatrix<double>, LocalVector<double>, double>     ls;
    Jacobi<LocalMatrix<double>, LocalVector<double>, double> pc;
    ls.SetOperator(mat);
    ls.SetPreconditioner(pc);
    ls.Build();
    ls.Verbose(0);
    ls.Solve(rhs, &x);
    const int    iters  = ls.GetIterationCount();
    const int    status = ls.GetSolverStatus();
    const double res    = ls.GetCurrentResidual();
    ls.Clear();
    e.ScaleAdd(-1.0, x);
    std::cout.precision(17);
    std::cout << "RESULT ptr_bytes=" << sizeof(PtrType) << " iters=" << iters << " status=" << status << " residual=" << res
              << " error=" << e.Norm() << std::endl;
    stop_rocalution();
    return 0;
}
