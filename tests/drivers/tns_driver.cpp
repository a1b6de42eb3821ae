// A driver as one would write it against the reference: CG preconditioned with TNS, for double and for float, in the
// implicit and in the explicit mode.  Compiled with plain g++ (tests/test_cpu_tns.py); running it needs the accelerator.
#include <rocalution/rocalution.hpp>

using namespace rocalution;

template <typename T>
static int run(const LocalMatrix<T>& mat, bool implicit, unsigned int format)
{
    LocalVector<T> x, rhs, e;
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    rhs.Allocate("rhs", mat.GetM());
    e.Allocate("e", mat.GetN());
    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();

    CG<LocalMatrix<T>, LocalVector<T>, T>  ls;
    TNS<LocalMatrix<T>, LocalVector<T>, T> p;
    p.Set(implicit);
    if(format != CSR)
        p.SetPrecondMatrixFormat(format);
    ls.SetOperator(mat);
    ls.SetPreconditioner(p);
    ls.Build();
    p.Print();
    ls.Solve(rhs, &x);
    const int iterations = ls.GetIterationCount();
    ls.Clear();
    return iterations;
}

int main(int argc, char* argv[])
{
    if(argc < 2)
        return 2;
    init_rocalution();
    int total = 0;
    {
        LocalMatrix<double> A;
        A.ReadFileMTX(argv[1]);
        A.MoveToAccelerator();
        total += run<double>(A, true, CSR) + run<double>(A, false, ELL);
    }
    {
        LocalMatrix<float> A;
        A.ReadFileMTX(argv[1]);
        A.MoveToAccelerator();
        total += run<float>(A, true, ELL) + run<float>(A, false, CSR);
    }
    stop_rocalution();
    return total > 0 ? 0 : 1;
}
