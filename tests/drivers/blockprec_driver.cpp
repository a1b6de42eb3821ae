// A driver as one would write it against the reference: GMRES preconditioned with the BlockPreconditioner (three blocks
// n/3, n/3, rest, ILU(0) on every diagonal block), and FGMRES with a VariablePreconditioner that goes round Jacobi,
// MultiColoredSGS and ILU.  Compiled with plain g++ (tests/test_cpu_blockprec.py); running it needs the accelerator.
//   blockprec_driver <matrix.mtx> <basis> <mode> [form: -1 | 0 | 1]
// mode: block | blockdiag | variable  -- one RESULT line (iterations, status, residual, the error against x = 1, the form
//                                        the preconditioner took; -1 for variable) and the residual history, HIST lines
//       extlast  -- one apply with the last diagonal block replaced by a copy of itself (SetExternalLastMatrix) against one
//                   without, and one after SetDiagonalSolver() + SetLSolver() against the default: CHECK lines, same=1
//       extbad   -- SetExternalLastMatrix with the whole operator: Build() stops
#include <rocalution/rocalution.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

using namespace rocalution;

typedef LocalMatrix<double> Mat;
typedef LocalVector<double> Vec;

static void report(IterativeLinearSolver<Mat, Vec, double>& ls, Vec& e, const Vec& x, int form)
{
    e.ScaleAdd(-1.0, x);
    printf("RESULT iters=%d status=%d residual=%.17g error=%.6e form=%d\n", ls.GetIterationCount(), ls.GetSolverStatus(),
           ls.GetCurrentResidual(), e.Norm(), form);
    const std::vector<double>& hist = ls.GetResidualHistory();
    for(size_t k = 0; k < hist.size(); ++k)
        printf("HIST %.17g\n", hist[k]);
}

static std::vector<double> apply(BlockPreconditioner<Mat, Vec, double>& bp, const Mat& mat, const Vec& rhs)
{
    Vec x;
    x.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    bp.SetOperator(mat);
    bp.Build();
    bp.Solve(rhs, &x);
    std::vector<double> out((size_t)mat.GetN());
    x.CopyToData(out.data());
    bp.Clear();
    return out;
}

int main(int argc, char* argv[])
{
    if(argc < 4)
    {
        std::cerr << argv[0] << " <matrix.mtx> <basis> <block | blockdiag | variable | extlast | extbad> [form]" << std::endl;
        return 2;
    }
    const int         basis = atoi(argv[2]);
    const std::string mode  = argv[3];
    const int         form  = argc > 4 ? atoi(argv[4]) : -1;
    init_rocalution();

    Mat mat;
    mat.ReadFileMTX(argv[1]);
    mat.MoveToAccelerator();
    Vec x, rhs, e;
    x.MoveToAccelerator();
    rhs.MoveToAccelerator();
    e.MoveToAccelerator();
    x.Allocate("x", mat.GetN());
    rhs.Allocate("rhs", mat.GetM());
    e.Allocate("e", mat.GetN());
    e.Ones();
    mat.Apply(e, &rhs);
    x.Zeros();

    const int nn    = (int)mat.GetM();
    const int sz[3] = {nn / 3, nn / 3, nn - 2 * (nn / 3)};

    if(mode == "block" || mode == "blockdiag")
    {
        GMRES<Mat, Vec, double>               ls;
        BlockPreconditioner<Mat, Vec, double> bp;
        ILU<Mat, Vec, double>                 loc[3];
        Solver<Mat, Vec, double>*             list[3] = {&loc[0], &loc[1], &loc[2]};
        bp.Set(3, sz, list);
        if(mode == "blockdiag")
            bp.SetDiagonalSolver();
        bp.SetForm(form);
        ls.SetOperator(mat);
        ls.SetPreconditioner(bp);
        ls.SetBasisSize(basis);
        ls.Verbose(0);
        ls.Build();
        bp.Print();
        ls.RecordResidualHistory();
        ls.Solve(rhs, &x);
        int64_t info[8];
        bp.GetInfo(info);
        report(ls, e, x, (int)info[0]);
        ls.Clear();
    }
    else if(mode == "variable")
    {
        // a different preconditioner on every application, round robin (flexible GMRES)
        FGMRES<Mat, Vec, double>                 ls;
        VariablePreconditioner<Mat, Vec, double> vp;
        Jacobi<Mat, Vec, double>                 v0;
        MultiColoredSGS<Mat, Vec, double>        v1;
        ILU<Mat, Vec, double>                    v2;
        Solver<Mat, Vec, double>*                list[3] = {&v0, &v1, &v2};
        vp.SetPreconditioner(3, list);
        ls.SetOperator(mat);
        ls.SetPreconditioner(vp);
        ls.SetBasisSize(basis);
        ls.Verbose(0);
        ls.Build();
        vp.Print();
        ls.RecordResidualHistory();
        ls.Solve(rhs, &x);
        report(ls, e, x, -1);
        ls.Clear();
    }
    else if(mode == "extlast")
    {
        std::vector<std::vector<double>> out;
        for(int variant = 0; variant < 4; ++variant) // plain | external copy of the last block | plain | diagonal, then L again
        {
            BlockPreconditioner<Mat, Vec, double> bp;
            ILU<Mat, Vec, double>                 loc[3];
            Solver<Mat, Vec, double>*             list[3] = {&loc[0], &loc[1], &loc[2]};
            bp.Set(3, sz, list);
            bp.SetForm(form);
            Mat last;
            if(variant == 1)
            {
                last.MoveToAccelerator();
                mat.ExtractSubMatrix(2 * (nn / 3), 2 * (nn / 3), sz[2], sz[2], &last);
                bp.SetExternalLastMatrix(last);
            }
            if(variant == 3)
            {
                bp.SetDiagonalSolver();
                bp.SetLSolver();
            }
            out.push_back(apply(bp, mat, rhs));
        }
        const size_t bytes = out[0].size() * sizeof(double);
        printf("CHECK extlast same=%d\n", memcmp(out[0].data(), out[1].data(), bytes) == 0 ? 1 : 0);
        printf("CHECK lsolver same=%d\n", memcmp(out[2].data(), out[3].data(), bytes) == 0 ? 1 : 0);
        double s = 0.0;
        for(double v : out[0])
            s += v * v;
        printf("CHECK norm2=%.17g\n", s);
    }
    else if(mode == "extbad")
    {
        BlockPreconditioner<Mat, Vec, double> bp;
        ILU<Mat, Vec, double>                 loc[3];
        Solver<Mat, Vec, double>*             list[3] = {&loc[0], &loc[1], &loc[2]};
        bp.Set(3, sz, list);
        bp.SetExternalLastMatrix(mat); // n x n where the last block is (n - 2 (n / 3)) square
        bp.SetOperator(mat);
        bp.Build(); // stops
        printf("CHECK extbad built\n");
    }
    else
    {
        std::cerr << "unknown mode " << mode << std::endl;
        return 2;
    }
    stop_rocalution();
    return 0;
}
