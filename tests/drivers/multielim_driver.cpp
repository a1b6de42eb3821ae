// A driver as one would write it against the reference: CG preconditioned with MultiElimination around MultiColoredILU(0),
// two levels and a drop-off tolerance.  Compiled with plain g++ (tests/test_cpu_multielim.py); running it needs the
// accelerator.
//   multielim_driver <matrix.mtx> [drop_off] [level] [format: csr | ell] [form: -1 | 0 | 1] [apply <rhs.bin> <x.bin>]
// It prints one RESULT line (iterations, status, residual, the error against x = 1, the diagonal-block sizes) and the
// residual history, HIST lines.  With "apply", the last-block solver is Jacobi and x = M^-1 rhs of the preconditioner alone
// is written to x.bin (doubles in, doubles out).  form goes to SetForm (1: the fused apply; an ELL request overrides it at the
// first level); FORMS lists the form each level took.
#include <rocalution/rocalution.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

using namespace rocalution;

int main(int argc, char* argv[])
{
    if(argc < 2)
    {
        std::cerr << argv[0] << " <matrix.mtx> [drop_off] [level] [format] [form] [apply <rhs.bin> <x.bin>]" << std::endl;
        return 2;
    }
    const double drop   = argc > 2 ? atof(argv[2]) : 0.4;
    const int    level  = argc > 3 ? atoi(argv[3]) : 2;
    const bool   ell    = argc > 4 && strcmp(argv[4], "ell") == 0;
    const int    form   = argc > 5 ? atoi(argv[5]) : -1;
    const bool   apply  = argc > 8 && strcmp(argv[6], "apply") == 0;
    init_rocalution();

    LocalMatrix<double> mat;
    LocalVector<double> x, rhs, e;
    mat.ReadFileMTX(argv[1]);
    mat.MoveToAccelerator();
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    rhs.Allocate("rhs", mat.GetM());
    e.Allocate("e", mat.GetN());

    MultiElimination<LocalMatrix<double>, LocalVector<double>, double> p;
    MultiColoredILU<LocalMatrix<double>, LocalVector<double>, double>  mcilu_p;
    Jacobi<LocalMatrix<double>, LocalVector<double>, double>           jacobi_p;
    if(ell)
        p.SetPrecondMatrixFormat(ELL);
    p.SetForm(form);

    if(apply)
    {
        const size_t        n = (size_t)mat.GetM();
        std::vector<double> h(n);
        std::ifstream       in(argv[7], std::ios::binary);
        in.read(reinterpret_cast<char*>(h.data()), sizeof(double) * n);
        rhs.CopyFromData(h.data());
        p.Set(jacobi_p, level, drop);
        p.SetOperator(mat);
        p.Build();
        p.Print();
        printf("FORMS");
        for(const MultiElimination<LocalMatrix<double>, LocalVector<double>, double>* q = &p; q != NULL; q = q->GetNextLevel())
        {
            int64_t info[8];
            q->GetInfo(info);
            printf(" %d", (int)info[0]);
        }
        printf("\n");
        p.Solve(rhs, &x);
        x.CopyToData(h.data());
        std::ofstream out(argv[8], std::ios::binary);
        out.write(reinterpret_cast<const char*>(h.data()), sizeof(double) * n);
        p.Clear();
        stop_rocalution();
        return 0;
    }

    mcilu_p.Set(0);
    p.Set(mcilu_p, level, drop);

    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();

    CG<LocalMatrix<double>, LocalVector<double>, double> cg;
    cg.SetOperator(mat);
    cg.SetPreconditioner(p);
    cg.Verbose(0);
    cg.Build();
    p.Print();
    cg.RecordResidualHistory();
    cg.Solve(rhs, &x);

    e.ScaleAdd(-1.0, x);
    const double error = e.Norm();
    const MultiElimination<LocalMatrix<double>, LocalVector<double>, double>* next = p.GetNextLevel();
    printf("RESULT iters=%d status=%d residual=%.17g error=%.6e size0=%d size1=%d\n", cg.GetIterationCount(), cg.GetSolverStatus(),
           cg.GetCurrentResidual(), error, p.GetSizeDiagBlock(), next ? next->GetSizeDiagBlock() : -1);
    const std::vector<double>& hist = cg.GetResidualHistory();
    for(size_t k = 0; k < hist.size(); ++k)
        printf("HIST %.17g\n", hist[k]);
    cg.Clear();
    stop_rocalution();
    return 0;
}
