// A driver as one would write it against the reference: GMRES preconditioned with additive Schwarz, three blocks with an
// overlap of four rows and ILU(0) on every block.  Compiled with plain g++ (tests/test_cpu_schwarz.py); running it needs
// the accelerator.
//   schwarz_driver <matrix.mtx> [basis] [ras] [form: -1 | 0 | 1 | 2]
// It prints one RESULT line (iterations, status, residual, the error against x = 1, the form the preconditioner took) and
// the residual history, HIST lines.  "ras" as third argument runs RAS instead of AS; form goes to SetForm.
#include <rocalution/rocalution.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

using namespace rocalution;

template <class P>
static int run(P& p, LocalMatrix<double>& mat, int basis, int form)
{
    LocalVector<double> x, rhs, e;
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    rhs.Allocate("rhs", mat.GetM());
    e.Allocate("e", mat.GetN());

    ILU<LocalMatrix<double>, LocalVector<double>, double>     loc[3];
    Solver<LocalMatrix<double>, LocalVector<double>, double>* list[3] = {&loc[0], &loc[1], &loc[2]};
    p.Set(3, 4, list);
    p.SetForm(form);

    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();

    GMRES<LocalMatrix<double>, LocalVector<double>, double> ls;
    ls.SetOperator(mat);
    ls.SetPreconditioner(p);
    ls.SetBasisSize(basis);
    ls.Verbose(0);
    ls.Build();
    p.Print();
    ls.RecordResidualHistory();
    ls.Solve(rhs, &x);

    e.ScaleAdd(-1.0, x);
    const double error = e.Norm();
    int64_t      info[8];
    p.GetInfo(info);
    printf("RESULT iters=%d status=%d residual=%.17g error=%.6e form=%d\n", ls.GetIterationCount(), ls.GetSolverStatus(),
           ls.GetCurrentResidual(), error, (int)info[0]);
    const std::vector<double>& hist = ls.GetResidualHistory();
    for(size_t k = 0; k < hist.size(); ++k)
        printf("HIST %.17g\n", hist[k]);
    ls.Clear();
    return 0;
}

int main(int argc, char* argv[])
{
    if(argc < 2)
    {
        std::cerr << argv[0] << " <matrix.mtx> [basis] [as | ras] [form]" << std::endl;
        return 2;
    }
    const int  basis = argc > 2 ? atoi(argv[2]) : 30;
    const bool ras   = argc > 3 && strcmp(argv[3], "ras") == 0;
    const int  form  = argc > 4 ? atoi(argv[4]) : -1;
    init_rocalution();

    LocalMatrix<double> mat;
    mat.ReadFileMTX(argv[1]);
    mat.MoveToAccelerator();
    int rc = 0;
    if(ras)
    {
        RAS<LocalMatrix<double>, LocalVector<double>, double> p;
        rc = run(p, mat, basis, form);
    }
    else
    {
        AS<LocalMatrix<double>, LocalVector<double>, double> p;
        rc = run(p, mat, basis, form);
    }
    stop_rocalution();
    return rc;
}
