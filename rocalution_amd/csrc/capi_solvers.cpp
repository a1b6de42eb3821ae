// capi_solvers.cpp -- C handles onto the compiled C++ API layer (include/rocalution/*.hpp).
// Host-only translation unit: it instantiates Solver<LocalMatrix,LocalVector> and
// Solver<GlobalMatrix,GlobalVector> exactly as a reference driver would (clients/samples/cg.cpp,
// gmres.cpp, bicgstab.cpp, mixed-precision.cpp, cg_mpi.cpp, bicgstab_mpi.cpp) and exposes
// Build()/Solve() through the flat C ABI for Python / C callers.
#include <memory>
#include <stdexcept>

// fatal errors of the C++ layer unwind as rocalution::fatal_error here (instead of exit(1), the reference's convention for
// its own drivers) and reach the caller as an error status: a Python process survives a missing file or a mismatched vector
#define RAMD_FATAL_THROWS
#include "../../include/rocalution/rocalution.hpp"

using namespace rocalution;

namespace
{

// argument errors that can be detected up front are reported through the status code; everything else the C++ layer calls
// fatal arrives as an exception at GUARD_END

struct SolverBase
{
    virtual ~SolverBase() {}
    virtual void init(double a, double r, double d, int mn, int mx) = 0;
    virtual void init_inner(double, double, double, int) {}
    virtual void set_basis(int) {}
    virtual void set_fused(bool)                                         = 0;
    virtual void set_verbose(int)                                        = 0;
    virtual void set_precond_format(int) {}
    virtual void set_decomposition(bool) {}
    virtual void set_fused_sweeps(bool) {}
    virtual void set_seed(unsigned long long) {}
    virtual void set_params(double, double) {}
    virtual void set_tri_solver(int, int, double, int) {}
    virtual void set_precond_params(double, double, double) {}
    virtual bool rebuild_numeric()
    {
        return false;
    }
    virtual int  precond_kind() const                                    = 0; // RAMD_PC_*
    virtual void set_precond_form(int) {}
    virtual void set_precond_local_params(double, double, double) {}
    virtual bool set_precond_blocks(const int*, int)
    {
        return false;
    }
    virtual bool set_precond_perm(ramd_vec_t)
    {
        return false;
    }
    virtual bool precond_info(int64_t*)
    {
        return false;
    }
    virtual void build(ramd_mat_t op)                                    = 0;
    virtual void solve(ramd_vec_t rhs, ramd_vec_t x)                     = 0;
    virtual bool is_built() const                                        = 0;
    virtual int  vec_dtype() const                                       = 0; // dtype of rhs / x
    virtual int  op_dtype() const                                        = 0; // dtype of the operator
    virtual int64_t op_rows() const                                      = 0; // rows of the operator Build() saw
    virtual bool precond_apply(ramd_vec_t, ramd_vec_t)                   = 0;
    virtual void result(int* it, int* st, double* res)                   = 0;
    virtual void   set_time_mark(int iteration)                          = 0;
    virtual double seconds_since_time_mark()                             = 0;
    virtual const std::vector<double>& history()                         = 0;
    virtual int                        num_colors()
    {
        return 0;
    }
    virtual void clear() = 0;
};

template <typename T>
struct Precs
{
    typedef LocalMatrix<T> M;
    typedef LocalVector<T> V;
    Jacobi<M, V, T>          jacobi;
    ILU<M, V, T>             ilu;
    MultiColoredSGS<M, V, T> mcsgs;
    MultiColoredGS<M, V, T>  mcgs;
    MultiColoredILU<M, V, T> mcilu;
    GS<M, V, T>              gs;
    SGS<M, V, T>             sgs;
    IC<M, V, T>              ic;
    UAAMG<M, V, T>           uaamg;
    SAAMG<M, V, T>           saamg;
    TNS<M, V, T>             tns;
    RugeStuebenAMG<M, V, T>  rsamg;
    MultiElimination<M, V, T> me;
    int                      me_level = 1, me_last = RAMD_PC_JACOBI; // handed to MultiElimination::Set before a build
    double                   me_drop  = 0.0;
    bool                     me_fmt_on = false;
    unsigned                 me_fmt    = CSR;
    AS<M, V, T>              as;
    RAS<M, V, T>             ras;
    int                      as_nb = 1, as_ov = 0, as_local = RAMD_PC_JACOBI, as_form = -1; // handed to AS::Set / SetForm before a build
    bool                     as_lp_on = false;
    double                   as_lp[3] = {0.0, 0.0, 0.0};
    std::vector<std::unique_ptr<Precs<T>>>        as_tables; // one table per block: its object of kind as_local is the block's solver
    std::vector<Solver<M, V, T>*>                 as_list;
    BlockPreconditioner<M, V, T> bp; // blocks, permutation and diagonal flag go to it before a build; local kind / form / local params: as_*
    std::vector<int>             bp_sizes;
    LocalVector<int>             bp_perm;
    bool                         bp_diag = false;
    Precs()
    {
        // the aggregation runs on the device with the PMIS strategy (the Greedy default is a sequential host sweep)
        uaamg.SetCoarseningStrategy(PMIS);
        saamg.SetCoarseningStrategy(PMIS);
        uaamg.Verbose(0);
        saamg.Verbose(0);
        rsamg.Verbose(0); // (the class's defaults stay: Greedy, Direct; ramd_solver_set_precond_params changes them)
    }
    Solver<M, V, T>*         get(int kind)
    {
        switch(kind)
        {
        case RAMD_PC_UAAMG:
            return &uaamg;
        case RAMD_PC_SAAMG:
            return &saamg;
        case RAMD_PC_GS:
            return &gs;
        case RAMD_PC_SGS:
            return &sgs;
        case RAMD_PC_IC:
            return &ic;
        case RAMD_PC_JACOBI:
            return &jacobi;
        case RAMD_PC_ILU0:
            return &ilu;
        case RAMD_PC_MCSGS:
            return &mcsgs;
        case RAMD_PC_MCGS:
            return &mcgs;
        case RAMD_PC_MCILU:
            return &mcilu;
        case RAMD_PC_TNS:
            return &tns;
        case RAMD_PC_RSAMG:
            return &rsamg;
        case RAMD_PC_MULTIELIM:
            me_arm(); // (the table's settings go to the object whenever it is handed out unbuilt)
            return &me;
        case RAMD_PC_AS:
            as_arm(&as);
            return &as;
        case RAMD_PC_RAS:
            as_arm(&ras);
            return &ras;
        case RAMD_PC_BLOCK:
            bp_arm();
            return &bp;
        default:
            return NULL;
        }
    }
    void me_arm()
    {
        if(me.IsBuilt())
            return;
        me.Set(*get(me_last), me_level, me_drop);
        if(me_fmt_on)
            me.SetPrecondMatrixFormat(me_fmt);
    }
    void as_arm(AS<M, V, T>* obj)
    {
        if(obj->IsBuilt())
            return;
        as_tables.clear();
        as_list.clear();
        for(int i = 0; i < as_nb; ++i)
        {
            as_tables.emplace_back(new Precs<T>);
            if(as_lp_on)
                as_tables.back()->set_params(as_local, as_lp[0], as_lp[1], as_lp[2]);
            as_list.push_back(as_tables.back()->get(as_local));
        }
        obj->Set(as_nb, as_ov, as_list.data());
        obj->SetForm(as_form);
    }
    void bp_arm()
    {
        if(bp.IsBuilt())
            return;
        if(bp_sizes.empty())
        {
            ramd_set_last_error("BlockPreconditioner: no block sizes (ramd_solver_set_precond_blocks) before the build");
            throw std::runtime_error("BlockPreconditioner: no block sizes (ramd_solver_set_precond_blocks) before the build");
        }
        as_tables.clear();
        as_list.clear();
        for(size_t i = 0; i < bp_sizes.size(); ++i)
        {
            as_tables.emplace_back(new Precs<T>);
            if(as_lp_on)
                as_tables.back()->set_params(as_local, as_lp[0], as_lp[1], as_lp[2]);
            as_list.push_back(as_tables.back()->get(as_local));
        }
        bp.Set((int)bp_sizes.size(), bp_sizes.data(), as_list.data());
        bp_diag ? bp.SetDiagonalSolver() : bp.SetLSolver();
        if(bp_perm.GetSize() > 0)
            bp.SetPermutation(bp_perm);
        bp.SetForm(as_form > 1 ? -1 : as_form);
    }
    // the parameters of ramd_solver_set_precond_params / ramd_gsolver_set_precond_params for the object of `pc_kind`
    void set_params(int pc_kind, double p0, double p1, double p2)
    {
        if(pc_kind == RAMD_PC_ILU0) // ILU::Set(p, level)
            ilu.Set((int)p0, p1 != 0.0);
        else if(pc_kind == RAMD_PC_TNS) // TNS::Set(imp), and the form of the implicit mode
        {
            tns.Set(p0 != 0.0);
            tns.SetForm((int)p1);
        }
        else if(pc_kind == RAMD_PC_RSAMG) // threshold; strategy + 2 interpolation + 4 FF1; rows of the coarsest level
        {
            const int bits = (int)p1;
            rsamg.SetStrengthThreshold((float)p0);
            rsamg.SetCoarseningStrategy((bits & 1) ? PMIS : Greedy);
            rsamg.SetInterpolationType((bits & 2) ? ExtPI : Direct);
            rsamg.SetInterpolationFF1Limit((bits & 4) != 0);
            if(p2 > 0.0)
                rsamg.SetCoarsestLevel((int)p2);
        }
        else if(pc_kind == RAMD_PC_MULTIELIM) // level, drop-off, kind of the last-block solver
        {
            me_level = (int)p0;
            me_drop  = p1;
            me_last  = (int)p2;
        }
        else if(pc_kind == RAMD_PC_AS || pc_kind == RAMD_PC_RAS) // blocks, overlap, kind of the local solvers
        {
            as_nb    = (int)p0;
            as_ov    = (int)p1;
            as_local = (int)p2;
        }
        else if(pc_kind == RAMD_PC_BLOCK) // diagonal solve, -, kind of the block solvers
        {
            bp_diag  = p0 != 0.0;
            as_local = (int)p2;
        }
    }
    void set_format(int pc_kind, int f)
    {
        if(pc_kind == RAMD_PC_TNS)
            tns.SetPrecondMatrixFormat((unsigned)f);
        else if(pc_kind == RAMD_PC_MULTIELIM)
        {
            me_fmt_on = true;
            me_fmt    = (unsigned)f;
        }
        else
            mc(pc_kind)->SetPrecondMatrixFormat((unsigned)f);
    }
    MultiColored<M, V, T>* mc(int kind)
    {
        if(kind == RAMD_PC_MCGS)
            return &mcgs;
        if(kind == RAMD_PC_MCILU)
            return &mcilu;
        return &mcsgs;
    }
};

template <typename T>
struct LocalSolver : SolverBase
{
    typedef LocalMatrix<T> M;
    typedef LocalVector<T> V;
    int                                             solver_kind, pc_kind;
    CG<M, V, T>                                     cg;
    GMRES<M, V, T>                                  gmres;
    BiCGStab<M, V, T>                               bicg;
    FCG<M, V, T>                                    fcg;
    CR<M, V, T>                                     cr;
    FGMRES<M, V, T>                                 fgmres;
    BiCGStabl<M, V, T>                              bicgl;
    QMRCGStab<M, V, T>                              qmr;
    IDR<M, V, T>                                    idr;
    FixedPoint<M, V, T>                             fp;
    Chebyshev<M, V, T>                              cheb;
    Precs<T>                                        pcs;
    M                                               op; // non-owning view of the caller's matrix
    bool                                            built = false;
    LocalSolver(int s, int p)
        : solver_kind(s)
        , pc_kind(p)
    {
        ls()->Verbose(0);
        ls()->RecordResidualHistory();
    }
    IterativeLinearSolver<M, V, T>* ls()
    {
        switch(solver_kind)
        {
        case RAMD_SOLVER_GMRES:
            return &gmres;
        case RAMD_SOLVER_BICGSTAB:
            return &bicg;
        case RAMD_SOLVER_FCG:
            return &fcg;
        case RAMD_SOLVER_CR:
            return &cr;
        case RAMD_SOLVER_FGMRES:
            return &fgmres;
        case RAMD_SOLVER_BICGSTABL:
            return &bicgl;
        case RAMD_SOLVER_QMRCGSTAB:
            return &qmr;
        case RAMD_SOLVER_IDR:
            return &idr;
        case RAMD_SOLVER_FIXEDPOINT:
            return &fp;
        case RAMD_SOLVER_CHEBYSHEV:
            return &cheb;
        default:
            return &cg;
        }
    }
    void init(double a, double r, double d, int mn, int mx) override
    {
        ls()->Init(a, r, d, mn, mx);
    }
    void set_basis(int m) override
    {
        if(solver_kind == RAMD_SOLVER_BICGSTABL)
            bicgl.SetOrder(m);
        else if(solver_kind == RAMD_SOLVER_FGMRES)
            fgmres.SetBasisSize(m);
        else if(solver_kind == RAMD_SOLVER_IDR)
            idr.SetShadowSpace(m);
        else
            gmres.SetBasisSize(m);
    }
    void set_seed(unsigned long long seed) override
    {
        idr.SetRandomSeed(seed);
    }
    void set_params(double p0, double p1) override
    {
        if(solver_kind == RAMD_SOLVER_FIXEDPOINT)
        {
            fp.SetRelaxation((T)p0);
            if(p1 != 0.0)
                fp.FlagSmoother();
        }
        else if(solver_kind == RAMD_SOLVER_CHEBYSHEV)
            cheb.Set((T)p0, (T)p1);
    }
    void set_tri_solver(int alg, int max_iter, double tol, int use_tol) override
    {
        SolverDescr d;
        d.SetTriSolverAlg(alg ? TriSolverAlg_Iterative : TriSolverAlg_Default);
        d.SetIterativeSolverMaxIteration(max_iter);
        d.SetIterativeSolverTolerance(tol);
        if(use_tol)
            d.EnableIterativeSolverTolerance();
        else
            d.DisableIterativeSolverTolerance();
        if(Solver<LocalMatrix<T>, LocalVector<T>, T>* p = pcs.get(pc_kind))
            p->SetSolverDescriptor(d);
    }
    void set_precond_params(double p0, double p1, double p2) override
    {
        pcs.set_params(pc_kind, p0, p1, p2);
    }
    void set_precond_form(int form) override
    {
        pcs.as_form = form;
    }
    void set_precond_local_params(double p0, double p1, double p2) override
    {
        pcs.as_lp_on = true;
        pcs.as_lp[0] = p0;
        pcs.as_lp[1] = p1;
        pcs.as_lp[2] = p2;
    }
    bool set_precond_blocks(const int* sizes, int nb) override
    {
        pcs.bp_sizes.assign(sizes, sizes + nb);
        return true;
    }
    bool set_precond_perm(ramd_vec_t perm) override
    {
        pcs.bp_perm.Clear();
        if(perm)
        {
            LocalVector<int> view;
            view.AdoptDeviceHandle(perm);
            pcs.bp_perm.MoveToAccelerator();
            pcs.bp_perm.CopyFrom(view);
        }
        return true;
    }
    bool precond_info(int64_t* out8) override
    {
        if(built && pc_kind == RAMD_PC_BLOCK)
        {
            pcs.bp.GetInfo(out8);
            return true;
        }
        if(!built || (pc_kind != RAMD_PC_AS && pc_kind != RAMD_PC_RAS))
            return false;
        (pc_kind == RAMD_PC_AS ? &pcs.as : &pcs.ras)->GetInfo(out8);
        return true;
    }
    void set_fused(bool f) override
    {
        ls()->SetFused(f);
    }
    void set_verbose(int v) override
    {
        ls()->Verbose(v);
    }
    void set_precond_format(int f) override
    {
        pcs.set_format(pc_kind, f);
    }
    void set_decomposition(bool d) override
    {
        pcs.mc(pc_kind)->SetDecomposition(d);
    }
    void set_fused_sweeps(bool f) override
    {
        pcs.mc(pc_kind)->SetFusedSweeps(f);
    }
    int precond_kind() const override
    {
        return pc_kind;
    }
    void build(ramd_mat_t h) override
    {
        if(built)
            clear();
        op.AdoptDeviceHandle(h);
        ls()->SetOperator(op);
        if(Solver<M, V, T>* p = pcs.get(pc_kind))
            ls()->SetPreconditioner(*p);
        ls()->Build();
        built = true;
    }
    void solve(ramd_vec_t rhs, ramd_vec_t x) override
    {
        V vr, vx;
        vr.AdoptDeviceHandle(rhs);
        vx.AdoptDeviceHandle(x);
        ls()->Solve(vr, &vx);
    }
    bool is_built() const override
    {
        return built;
    }
    int vec_dtype() const override
    {
        return sizeof(T) == 8 ? RAMD_F64 : RAMD_F32;
    }
    int op_dtype() const override
    {
        return vec_dtype();
    }
    int64_t op_rows() const override
    {
        return op.GetM();
    }
    bool precond_apply(ramd_vec_t rhs, ramd_vec_t x) override
    {
        if(!built)
            return false;
        Solver<M, V, T>* p = pcs.get(pc_kind);
        if(!p)
            return false;
        V vr, vx;
        vr.AdoptDeviceHandle(rhs);
        vx.AdoptDeviceHandle(x);
        p->SolveZeroSol(vr, &vx);
        return true;
    }
    void result(int* it, int* st, double* res) override
    {
        *it  = ls()->GetIterationCount();
        *st  = ls()->GetSolverStatus();
        *res = ls()->GetCurrentResidual();
    }
    void set_time_mark(int iteration) override
    {
        ls()->SetTimeMark(iteration);
    }
    double seconds_since_time_mark() override
    {
        return ls()->GetSecondsSinceTimeMark();
    }
    const std::vector<double>& history() override
    {
        return ls()->GetResidualHistory();
    }
    int num_colors() override
    {
        return pcs.mc(pc_kind)->GetNumColors();
    }
    void clear() override
    {
        if(built)
            ls()->Clear(); // also clears (and detaches) the preconditioner, like the reference
        built = false;
    }
    bool rebuild_numeric() override
    {
        if(!built)
            return false;
        ls()->ReBuildNumeric();
        return true;
    }
};

struct MixedSolver : SolverBase
{
    typedef LocalMatrix<double> MH;
    typedef LocalVector<double> VH;
    typedef LocalMatrix<float>  ML;
    typedef LocalVector<float>  VL;
    MixedPrecisionDC<MH, VH, double, ML, VL, float> mp;
    int                                             inner_kind, pc_kind;
    CG<ML, VL, float>                               cg;
    GMRES<ML, VL, float>                            gmres;
    BiCGStab<ML, VL, float>                         bicg;
    Precs<float>                                    pcs;
    MH                                              op;
    bool                                            built = false;
    MixedSolver(int s, int p)
        : inner_kind(s)
        , pc_kind(p)
    {
        mp.Verbose(0);
        mp.RecordResidualHistory();
        inner()->Verbose(0);
    }
    IterativeLinearSolver<ML, VL, float>* inner()
    {
        if(inner_kind == RAMD_SOLVER_GMRES)
            return &gmres;
        if(inner_kind == RAMD_SOLVER_BICGSTAB)
            return &bicg;
        return &cg;
    }
    void init(double a, double r, double d, int mn, int mx) override
    {
        mp.Init(a, r, d, mn, mx);
    }
    void init_inner(double a, double r, double d, int mx) override
    {
        inner()->Init(a, r, d, mx);
    }
    void set_basis(int m) override
    {
        gmres.SetBasisSize(m);
    }
    void set_fused(bool f) override
    {
        inner()->SetFused(f);
    }
    void set_verbose(int v) override
    {
        mp.Verbose(v);
    }
    int precond_kind() const override
    {
        return pc_kind;
    }
    void build(ramd_mat_t h) override
    {
        if(built)
            clear();
        op.AdoptDeviceHandle(h);
        if(Solver<ML, VL, float>* p = pcs.get(pc_kind))
            inner()->SetPreconditioner(*p);
        mp.SetOperator(op);
        mp.Set(*inner());
        mp.Build();
        built = true;
    }
    void solve(ramd_vec_t rhs, ramd_vec_t x) override
    {
        VH vr, vx;
        vr.AdoptDeviceHandle(rhs);
        vx.AdoptDeviceHandle(x);
        mp.Solve(vr, &vx);
    }
    bool is_built() const override
    {
        return built;
    }
    int vec_dtype() const override
    {
        return RAMD_F64;
    }
    int op_dtype() const override
    {
        return RAMD_F64;
    }
    int64_t op_rows() const override
    {
        return op.GetM();
    }
    // the inner (fp32) preconditioner takes the same settings as a stand-alone solver's
    void set_tri_solver(int alg, int max_iter, double tol, int use_tol) override
    {
        SolverDescr d;
        d.SetTriSolverAlg(alg ? TriSolverAlg_Iterative : TriSolverAlg_Default);
        d.SetIterativeSolverMaxIteration(max_iter);
        d.SetIterativeSolverTolerance(tol);
        if(use_tol)
            d.EnableIterativeSolverTolerance();
        else
            d.DisableIterativeSolverTolerance();
        if(Solver<ML, VL, float>* p = pcs.get(pc_kind))
            p->SetSolverDescriptor(d);
    }
    void set_precond_params(double p0, double p1, double) override
    {
        if(pc_kind == RAMD_PC_ILU0) // ILU::Set(p, level)
            pcs.ilu.Set((int)p0, p1 != 0.0);
    }
    void set_precond_format(int f) override
    {
        pcs.mc(pc_kind)->SetPrecondMatrixFormat((unsigned)f);
    }
    void set_decomposition(bool d) override
    {
        pcs.mc(pc_kind)->SetDecomposition(d);
    }
    void set_fused_sweeps(bool f) override
    {
        pcs.mc(pc_kind)->SetFusedSweeps(f);
    }
    bool precond_apply(ramd_vec_t, ramd_vec_t) override
    {
        return false;
    }
    void result(int* it, int* st, double* res) override
    {
        *it  = mp.GetIterationCount();
        *st  = mp.GetSolverStatus();
        *res = mp.GetCurrentResidual();
    }
    void set_time_mark(int iteration) override
    {
        mp.SetTimeMark(iteration);
    }
    double seconds_since_time_mark() override
    {
        return mp.GetSecondsSinceTimeMark();
    }
    const std::vector<double>& history() override
    {
        return mp.GetResidualHistory();
    }
    void clear() override
    {
        if(built)
            mp.Clear();
        built = false;
    }
};

} // namespace

struct ramd_solver_s
{
    std::unique_ptr<SolverBase> impl;
};

// ------------------------------------------------------------------------------------ distributed
struct ramd_gsolver_s
{
    typedef GlobalMatrix<double> GM;
    typedef GlobalVector<double> GV;
    typedef LocalMatrix<double>  LM;
    typedef LocalVector<double>  LV;
    ParallelManager              pm;
    GM                           A;
    GV                           x, rhs, tmp;
    int                          solver_kind, pc_kind;
    CG<GM, GV, double>           cg;
    GMRES<GM, GV, double>        gmres;
    BiCGStab<GM, GV, double>     bicg;
    Jacobi<GM, GV, double>       jacobi; // global Jacobi == interior diagonal
    BlockJacobi<GM, GV, double>  bj;
    Precs<double>                precs; // local preconditioners for BlockJacobi (any RAMD_PC_* kind)
    UAAMG<GM, GV, double>        guaamg; // aggregation AMG on the GlobalMatrix itself (RAMD_PC_GLOBAL_*)
    SAAMG<GM, GV, double>        gsaamg;
    // mixed precision: fp64 defect correction around an fp32 Global solver
    typedef GlobalMatrix<float>  GMF;
    typedef GlobalVector<float>  GVF;
    bool                         mixed = false;
    int                          inner_kind = RAMD_SOLVER_CG;
    MixedPrecisionDC<GM, GV, double, GMF, GVF, float> mp;
    CG<GMF, GVF, float>          cgf;
    GMRES<GMF, GVF, float>       gmresf;
    BiCGStab<GMF, GVF, float>    bicgf;
    Jacobi<GMF, GVF, float>      jacobif;
    bool                         setup = false, built = false;
    IterativeLinearSolver<GMF, GVF, float>* inner()
    {
        if(inner_kind == RAMD_SOLVER_GMRES)
            return &gmresf;
        if(inner_kind == RAMD_SOLVER_BICGSTAB)
            return &bicgf;
        return &cgf;
    }
    IterativeLinearSolver<GM, GV, double>* ls()
    {
        if(mixed)
            return &mp;
        if(solver_kind == RAMD_SOLVER_GMRES)
            return &gmres;
        if(solver_kind == RAMD_SOLVER_BICGSTAB)
            return &bicg;
        return &cg;
    }
    void alloc_vectors()
    {
        GV* vs[] = {&x, &rhs, &tmp};
        for(GV* v : vs)
        {
            v->SetParallelManager(pm);
            v->MoveToAccelerator();
            v->Allocate("v", pm.GetGlobalNrow());
        }
    }
};

#define GUARD_BEGIN try {
#define GUARD_END                                       \
    }                                                   \
    catch(const std::exception& e)                      \
    {                                                   \
        fprintf(stderr, "rocalution_amd: %s\n", e.what()); \
        ramd_set_last_error(e.what());                  \
        return RAMD_ERR_STATE;                          \
    }                                                   \
    return RAMD_OK;

template <typename T>
static void mat_file_io(ramd_mat_t h, const char* filename, int kind, bool read)
{
    LocalMatrix<T> m;
    m.AdoptDeviceHandle(h);
    if(read)
        kind == RAMD_FILE_MTX ? m.ReadFileMTX(filename) : m.ReadFileCSR(filename);
    else
        kind == RAMD_FILE_MTX ? m.WriteFileMTX(filename) : m.WriteFileCSR(filename);
}
template <typename T>
static void vec_file_io(ramd_vec_t h, const char* filename, int kind, bool read)
{
    LocalVector<T> v;
    v.AdoptDeviceHandle(h);
    if(read)
        kind == RAMD_FILE_ASCII ? v.ReadFileASCII(filename) : v.ReadFileBinary(filename);
    else
        kind == RAMD_FILE_ASCII ? v.WriteFileASCII(filename) : v.WriteFileBinary(filename);
}
extern "C" {

int ramd_solver_create(int solver, int precond, int dtype, ramd_solver_t* out)
{
    if(!out || solver < 0 || solver > RAMD_SOLVER_CHEBYSHEV || precond < 0
       || (precond > RAMD_PC_SAAMG && precond != RAMD_PC_TNS && precond != RAMD_PC_RSAMG && precond != RAMD_PC_MULTIELIM
           && precond != RAMD_PC_AS && precond != RAMD_PC_RAS && precond != RAMD_PC_BLOCK)
       || (dtype != RAMD_F64 && dtype != RAMD_F32))
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    ramd_solver_s* s = new ramd_solver_s;
    if(dtype == RAMD_F64)
        s->impl.reset(new LocalSolver<double>(solver, precond));
    else
        s->impl.reset(new LocalSolver<float>(solver, precond));
    *out = s;
    GUARD_END
}

int ramd_solver_create_mixed(int inner_solver, int inner_precond, ramd_solver_t* out)
{
    if(inner_precond == RAMD_PC_BLOCK)
    {
        ramd_set_last_error("solver_create_mixed: the BlockPreconditioner is not offered inside the mixed-precision driver");
        return RAMD_ERR_ARG;
    }
    if(!out || inner_solver < 0 || inner_solver > 2 || inner_precond < 0 || inner_precond > RAMD_PC_SAAMG)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    ramd_solver_s* s = new ramd_solver_s;
    s->impl.reset(new MixedSolver(inner_solver, inner_precond));
    *out = s;
    GUARD_END
}

int ramd_solver_destroy(ramd_solver_t s)
{
    if(s)
    {
        s->impl->clear();
        delete s;
    }
    return RAMD_OK;
}

int ramd_solver_init(ramd_solver_t s, double a, double r, double d, int mn, int mx)
{
    if(!s || mn < 0 || mx < mn)
        return RAMD_ERR_ARG;
    s->impl->init(a, r, d, mn, mx);
    return RAMD_OK;
}
int ramd_solver_init_inner(ramd_solver_t s, double a, double r, double d, int mx)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->init_inner(a, r, d, mx);
    return RAMD_OK;
}
int ramd_solver_set_params(ramd_solver_t s, double p0, double p1)
{
    if(!s)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    s->impl->set_params(p0, p1);
    GUARD_END
}
int ramd_solver_set_tri_solver(ramd_solver_t s, int iterative, int max_iter, double tol, int use_tol)
{
    if(!s || max_iter < 0)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    s->impl->set_tri_solver(iterative, max_iter, tol, use_tol);
    GUARD_END
}
// what ramd_solver_set_precond_params and ramd_gsolver_set_precond_params accept for a preconditioner kind
static int check_precond_params(int kind, double p0, double p1, double p2)
{
    if((kind == RAMD_PC_TNS && (p1 < -1.0 || p1 > 1.0 || p1 != (double)(int)p1))
       || (kind == RAMD_PC_RSAMG && (p1 < 0.0 || p1 > 7.0 || p1 != (double)(int)p1 || p2 < 0.0)))
        return RAMD_ERR_ARG;
    if(kind == RAMD_PC_MULTIELIM)
    {
        const int last = (int)p2;
        if(p0 < 0.0 || p0 != (double)(int)p0 || !(p1 >= 0.0) || p2 != (double)last)
        {
            ramd_set_last_error("MultiElimination: level (an integer >= 0), drop-off (>= 0) and the kind of the last-block solver expected");
            return RAMD_ERR_ARG;
        }
        if(last == RAMD_PC_MULTIELIM || last == RAMD_PC_UAAMG || last == RAMD_PC_SAAMG || last == RAMD_PC_RSAMG
           || last == RAMD_PC_GLOBAL_UAAMG || last == RAMD_PC_GLOBAL_SAAMG || last <= RAMD_PC_NONE || last > RAMD_PC_MULTIELIM
           || last == 15)
        {
            ramd_set_last_error("MultiElimination: the last-block solver is one of Jacobi, ILU, MultiColoredSGS / GS / ILU, GS, SGS, IC "
                                "or TNS; MultiElimination itself (its level sets the depth) and the AMG kinds are refused");
            return RAMD_ERR_ARG;
        }
    }
    if(kind == RAMD_PC_BLOCK)
    {
        const int local = (int)p2;
        if(p2 != (double)local
           || !(local == RAMD_PC_JACOBI || local == RAMD_PC_ILU0 || local == RAMD_PC_MCSGS || local == RAMD_PC_MCGS || local == RAMD_PC_MCILU
                || local == RAMD_PC_GS || local == RAMD_PC_SGS || local == RAMD_PC_IC || local == RAMD_PC_TNS))
        {
            ramd_set_last_error("BlockPreconditioner: the block solvers are one of Jacobi, ILU, MultiColoredSGS / GS / ILU, GS, SGS, IC or TNS");
            return RAMD_ERR_ARG;
        }
    }
    if(kind == RAMD_PC_AS || kind == RAMD_PC_RAS)
    {
        const int local = (int)p2;
        if(p0 != (double)(int)p0 || p1 != (double)(int)p1 || p2 != (double)local)
        {
            ramd_set_last_error("AS: the number of blocks, the overlap and the kind of the local solvers expected (integers)");
            return RAMD_ERR_ARG;
        }
        if(p0 < 1.0)
        {
            ramd_set_last_error("AS: the number of blocks must be at least 1");
            return RAMD_ERR_ARG;
        }
        if(p1 < 0.0)
        {
            ramd_set_last_error("AS: the overlap must not be negative");
            return RAMD_ERR_ARG;
        }
        if(!(local == RAMD_PC_JACOBI || local == RAMD_PC_ILU0 || local == RAMD_PC_MCSGS || local == RAMD_PC_MCGS || local == RAMD_PC_MCILU
             || local == RAMD_PC_GS || local == RAMD_PC_SGS || local == RAMD_PC_IC || local == RAMD_PC_TNS))
        {
            ramd_set_last_error("AS: the local solvers are one of Jacobi, ILU, MultiColoredSGS / GS / ILU, GS, SGS, IC or TNS");
            return RAMD_ERR_ARG;
        }
    }
    return RAMD_OK;
}
int ramd_solver_set_precond_form(ramd_solver_t s, int form)
{
    if(!s || (s->impl->precond_kind() != RAMD_PC_AS && s->impl->precond_kind() != RAMD_PC_RAS && s->impl->precond_kind() != RAMD_PC_BLOCK)
       || s->impl->is_built())
        return RAMD_ERR_ARG;
    if(s->impl->precond_kind() == RAMD_PC_BLOCK && (form < -1 || form > 1))
    {
        ramd_set_last_error("BlockPreconditioner: form is -1 (auto), 0 (stepwise) or 1 (fused)");
        return RAMD_ERR_ARG;
    }
    if(form < -1 || form > 2)
    {
        ramd_set_last_error("AS: form is -1 (auto), 0 (stepwise), 1 (fused) or 2 (stacked)");
        return RAMD_ERR_ARG;
    }
    s->impl->set_precond_form(form);
    return RAMD_OK;
}
int ramd_solver_set_precond_local_params(ramd_solver_t s, double p0, double p1, double p2)
{
    if(!s || (s->impl->precond_kind() != RAMD_PC_AS && s->impl->precond_kind() != RAMD_PC_RAS && s->impl->precond_kind() != RAMD_PC_BLOCK)
       || s->impl->is_built())
        return RAMD_ERR_ARG;
    s->impl->set_precond_local_params(p0, p1, p2);
    return RAMD_OK;
}
int ramd_solver_set_precond_blocks(ramd_solver_t s, const int* sizes, int nb)
{
    if(!s || s->impl->precond_kind() != RAMD_PC_BLOCK || s->impl->is_built())
        return RAMD_ERR_ARG;
    if(nb < 1 || !sizes)
    {
        ramd_set_last_error("BlockPreconditioner: the number of blocks must be at least 1");
        return RAMD_ERR_ARG;
    }
    for(int i = 0; i < nb; ++i)
        if(sizes[i] < 1)
        {
            ramd_set_last_error("BlockPreconditioner: every block needs at least one row");
            return RAMD_ERR_ARG;
        }
    GUARD_BEGIN
    if(!s->impl->set_precond_blocks(sizes, nb))
        return RAMD_ERR_ARG;
    GUARD_END
}
int ramd_solver_set_precond_perm(ramd_solver_t s, ramd_vec_t perm)
{
    if(!s || s->impl->precond_kind() != RAMD_PC_BLOCK || s->impl->is_built())
        return RAMD_ERR_ARG;
    int dtype = 0;
    if(perm && (ramd_vec_dtype(perm, &dtype) != RAMD_OK || dtype != RAMD_I32))
    {
        ramd_set_last_error("BlockPreconditioner: the permutation must be an int32 vector");
        return RAMD_ERR_ARG;
    }
    GUARD_BEGIN
    if(!s->impl->set_precond_perm(perm))
        return RAMD_ERR_ARG;
    GUARD_END
}
int ramd_solver_precond_info(ramd_solver_t s, int64_t* out8)
{
    if(!s || !out8)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    if(!s->impl->precond_info(out8))
    {
        ramd_set_last_error("solver_precond_info: an AS / RAS / BlockPreconditioner after Build() expected");
        return RAMD_ERR_STATE;
    }
    GUARD_END
}
int ramd_solver_set_precond_params(ramd_solver_t s, double p0, double p1, double p2)
{
    if(!s || check_precond_params(s->impl->precond_kind(), p0, p1, p2) != RAMD_OK)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    s->impl->set_precond_params(p0, p1, p2);
    GUARD_END
}
int ramd_solver_set_seed(ramd_solver_t s, unsigned long long seed)
{
    if(!s || seed == 0ULL)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    s->impl->set_seed(seed);
    GUARD_END
}
int ramd_solver_set_basis(ramd_solver_t s, int m)
{
    if(!s || m < 1)
        return RAMD_ERR_ARG;
    s->impl->set_basis(m);
    return RAMD_OK;
}
int ramd_solver_set_fused(ramd_solver_t s, int on)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_fused(on != 0);
    return RAMD_OK;
}
int ramd_solver_set_verbose(ramd_solver_t s, int v)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_verbose(v);
    return RAMD_OK;
}
int ramd_solver_set_precond_format(ramd_solver_t s, int f)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_precond_format(f);
    return RAMD_OK;
}
int ramd_solver_set_decomposition(ramd_solver_t s, int d)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_decomposition(d != 0);
    return RAMD_OK;
}
int ramd_solver_set_fused_sweeps(ramd_solver_t s, int on)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_fused_sweeps(on != 0);
    return RAMD_OK;
}
int ramd_mat_read_mtx(const char* filename, int dtype, ramd_mat_t* out)
{
    return ramd_mat_read_file(filename, RAMD_FILE_MTX, dtype, out);
}
int ramd_mat_read_file(const char* filename, int kind, int dtype, ramd_mat_t* out)
{
    if(!filename || !out || (dtype != RAMD_F64 && dtype != RAMD_F32) || (kind != 0 && kind != 1))
        return RAMD_ERR_ARG;
    ramd_mat_t h = NULL;
    if(ramd_mat_create(dtype, &h) != RAMD_OK)
        return RAMD_ERR_HIP;
    try
    {
        if(dtype == RAMD_F64)
            mat_file_io<double>(h, filename, kind, true);
        else
            mat_file_io<float>(h, filename, kind, true);
    }
    catch(const std::exception& e)
    {
        (void)ramd_mat_destroy(h);
        ramd_set_last_error((std::string("reading ") + filename + ": " + e.what()).c_str());
        return RAMD_ERR_STATE;
    }
    *out = h;
    return RAMD_OK;
}
int ramd_mat_write_file(ramd_mat_t m, const char* filename, int kind)
{
    int bits = 32;
    if(m && ramd_mat_ptr_bits(m, &bits) == RAMD_OK && bits == 64) // (the file formats hold 32-bit row offsets)
    {
        ramd_set_last_error("ramd_mat_write_file: not provided for 64-bit row offsets");
        return RAMD_ERR_UNSUPPORTED;
    }
    int dtype = 0;
    if(!m || !filename || (kind != 0 && kind != 1) || ramd_mat_info(m, NULL, NULL, NULL, NULL, &dtype) != RAMD_OK)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    if(dtype == RAMD_F64)
        mat_file_io<double>(m, filename, kind, false);
    else
        mat_file_io<float>(m, filename, kind, false);
    GUARD_END
}
static int vec_file(ramd_vec_t v, const char* filename, int kind, bool read)
{
    int dtype = 0;
    if(!v || !filename || (kind != 0 && kind != 1) || ramd_vec_dtype(v, &dtype) != RAMD_OK)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    if(dtype == RAMD_F64)
        vec_file_io<double>(v, filename, kind, read);
    else if(dtype == RAMD_F32)
        vec_file_io<float>(v, filename, kind, read);
    else
        vec_file_io<int>(v, filename, kind, read);
    GUARD_END
}
int ramd_vec_read_file(ramd_vec_t v, const char* filename, int kind)
{
    return vec_file(v, filename, kind, true);
}
int ramd_vec_write_file(ramd_vec_t v, const char* filename, int kind)
{
    return vec_file(v, filename, kind, false);
}
int ramd_solver_build(ramd_solver_t s, ramd_mat_t op)
{
    int nrow = 0, ncol = 0, dtype = 0;
    if(!s || !op || ramd_mat_info(op, &nrow, &ncol, NULL, NULL, &dtype) != RAMD_OK)
        return RAMD_ERR_ARG;
    if(dtype != s->impl->op_dtype())
    {
        ramd_set_last_error("solver_build: the operator's value type is not the solver's");
        return RAMD_ERR_ARG;
    }
    if(nrow != ncol)
    {
        ramd_set_last_error("solver_build: the operator is not square");
        return RAMD_ERR_ARG;
    }
    // an operator with 64-bit row offsets: Jacobi or no preconditioner; everything else is refused here, before Build() has
    // touched the solver (ILU, the multi-coloured sweeps, AMG ... would stop at their first matrix operation, half built)
    int bits = 32;
    if(ramd_mat_ptr_bits(op, &bits) == RAMD_OK && bits == 64 && s->impl->precond_kind() != RAMD_PC_NONE
       && s->impl->precond_kind() != RAMD_PC_JACOBI)
    {
        ramd_set_last_error("solver_build: this preconditioner is not provided for 64-bit row offsets (Jacobi or none)");
        return RAMD_ERR_UNSUPPORTED;
    }
    try
    {
        s->impl->build(op);
    }
    catch(const std::exception& e)
    {
        // a WIDE operator whose solver stopped at an entry that matrices with 64-bit row offsets do not provide: that refusal is
        // the answer, not the generic "fatal error" state (a narrow operator keeps RAMD_ERR_STATE whatever the text says)
        const std::string refused = ramd_last_error();
        fprintf(stderr, "rocalution_amd: %s\n", e.what());
        if(bits == 64 && refused.find("not provided for 64-bit row offsets") != std::string::npos)
        {
            ramd_set_last_error(("solver_build: " + refused).c_str());
            return RAMD_ERR_UNSUPPORTED;
        }
        // AS / RAS refuse a layout or a form with a text of their own ("AS: ..."): that text is the answer
        if((s->impl->precond_kind() == RAMD_PC_AS || s->impl->precond_kind() == RAMD_PC_RAS)
           && (refused.find("AS: ") != std::string::npos))
        {
            ramd_set_last_error(("solver_build: " + refused).c_str());
            return RAMD_ERR_ARG;
        }
        // ... and so does the BlockPreconditioner (sizes, permutation)
        if(s->impl->precond_kind() == RAMD_PC_BLOCK && refused.find("BlockPreconditioner: ") != std::string::npos)
        {
            ramd_set_last_error(("solver_build: " + refused).c_str());
            return RAMD_ERR_ARG;
        }
        ramd_set_last_error(e.what());
        return RAMD_ERR_STATE;
    }
    return RAMD_OK;
}
int ramd_solver_solve(ramd_solver_t s, ramd_vec_t rhs, ramd_vec_t x)
{
    if(!s || !rhs || !x || rhs == x)
        return RAMD_ERR_ARG;
    if(!s->impl->is_built())
    {
        ramd_set_last_error("solver_solve: Solve() before Build() (or after Clear())");
        return RAMD_ERR_STATE;
    }
    int     dr = 0, dx = 0;
    int64_t nr = 0, nx = 0;
    if(ramd_vec_dtype(rhs, &dr) != RAMD_OK || ramd_vec_dtype(x, &dx) != RAMD_OK || ramd_vec_size(rhs, &nr) != RAMD_OK
       || ramd_vec_size(x, &nx) != RAMD_OK)
        return RAMD_ERR_ARG;
    if(dr != s->impl->vec_dtype() || dx != dr || nr != s->impl->op_rows() || nx != nr)
    {
        ramd_set_last_error("solver_solve: rhs / x do not match the operator (value type or size)");
        return RAMD_ERR_ARG;
    }
    GUARD_BEGIN
    s->impl->solve(rhs, x);
    GUARD_END
}
int ramd_solver_precond_apply(ramd_solver_t s, ramd_vec_t rhs, ramd_vec_t x)
{
    if(!s || !rhs || !x || rhs == x)
        return RAMD_ERR_ARG;
    return s->impl->precond_apply(rhs, x) ? RAMD_OK : RAMD_ERR_STATE;
}
int ramd_solver_set_time_mark(ramd_solver_t s, int iteration)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->set_time_mark(iteration);
    return RAMD_OK;
}
int ramd_solver_seconds_since_time_mark(ramd_solver_t s, double* seconds)
{
    if(!s || !seconds)
        return RAMD_ERR_ARG;
    *seconds = s->impl->seconds_since_time_mark();
    return RAMD_OK;
}
int ramd_solver_result(ramd_solver_t s, int* iters, int* status, double* final_res)
{
    if(!s)
        return RAMD_ERR_ARG;
    int    it, st;
    double res;
    s->impl->result(&it, &st, &res);
    if(iters)
        *iters = it;
    if(status)
        *status = st;
    if(final_res)
        *final_res = res;
    return RAMD_OK;
}
int ramd_solver_history(ramd_solver_t s, double* buf, int cap, int* len)
{
    if(!s)
        return RAMD_ERR_ARG;
    const std::vector<double>& h = s->impl->history();
    if(len)
        *len = (int)h.size();
    for(int i = 0; i < cap && i < (int)h.size(); ++i)
        buf[i] = h[(size_t)i];
    return RAMD_OK;
}
int ramd_solver_num_colors(ramd_solver_t s, int* n)
{
    if(!s || !n)
        return RAMD_ERR_ARG;
    *n = s->impl->num_colors();
    return RAMD_OK;
}
int ramd_solver_rebuild_numeric(ramd_solver_t s)
{
    if(!s)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    if(!s->impl->rebuild_numeric())
        return RAMD_ERR_STATE;
    GUARD_END
}
int ramd_solver_clear(ramd_solver_t s)
{
    if(!s)
        return RAMD_ERR_ARG;
    s->impl->clear();
    return RAMD_OK;
}

// ------------------------------------------------------------------------------------ distributed
int ramd_gsolver_create(ramd_comm_t comm, int solver, int precond, ramd_gsolver_t* out)
{
    if(precond == RAMD_PC_BLOCK)
    {
        ramd_set_last_error("gsolver_create: the BlockPreconditioner is not provided on Global objects (not under BlockJacobi either)");
        return RAMD_ERR_ARG;
    }
    if(!out || solver < 0 || solver > 2 || precond < 0 || (precond > RAMD_PC_RSAMG && precond != RAMD_PC_MULTIELIM))
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    ramd_gsolver_s* g = new ramd_gsolver_s;
    g->solver_kind    = solver;
    g->pc_kind        = precond;
    g->pm.SetMPICommunicator(comm);
    g->ls()->Verbose(0);
    *out = g;
    GUARD_END
}

int ramd_gsolver_create_mixed(ramd_comm_t comm, int inner_solver, int inner_precond, ramd_gsolver_t* out)
{
    if(!out || inner_solver < 0 || inner_solver > 2
       || (inner_precond != RAMD_PC_NONE && inner_precond != RAMD_PC_JACOBI))
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    ramd_gsolver_s* g = new ramd_gsolver_s;
    g->mixed          = true;
    g->inner_kind     = inner_solver;
    g->solver_kind    = RAMD_SOLVER_CG;
    g->pc_kind        = inner_precond;
    g->pm.SetMPICommunicator(comm);
    g->mp.Verbose(0);
    g->inner()->Verbose(0);
    *out = g;
    GUARD_END
}
int ramd_gsolver_init_inner(ramd_gsolver_t g, double a, double r, double d, int mx)
{
    if(!g || !g->mixed)
        return RAMD_ERR_ARG;
    g->inner()->Init(a, r, d, mx);
    return RAMD_OK;
}
int ramd_gsolver_destroy(ramd_gsolver_t g)
{
    if(g)
    {
        if(g->built)
            g->ls()->Clear();
        delete g;
    }
    return RAMD_OK;
}

static int gsolver_setup_slab(ramd_gsolver_t g, int N, int z_begin, int z_end, bool lap27);
int ramd_gsolver_setup_poisson(ramd_gsolver_t g, int N, int z_begin, int z_end)
{
    return gsolver_setup_slab(g, N, z_begin, z_end, false);
}
int ramd_gsolver_setup_laplace27(ramd_gsolver_t g, int N, int z_begin, int z_end)
{
    return gsolver_setup_slab(g, N, z_begin, z_end, true);
}
// (both operators couple a plane to the planes next to it and to nothing else: one halo plan)
static int gsolver_setup_slab(ramd_gsolver_t g, int N, int z_begin, int z_end, bool lap27)
{
    if(!g || N < 1 || z_begin < 0 || z_end > N || z_begin >= z_end)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    const int64_t N2 = (int64_t)N * N, n = N2 * N;
    const int64_t lo = z_begin * N2, hi = z_end * N2, nloc = hi - lo;
    const int     rank = g->pm.GetRank(), np = g->pm.GetNumProcs();
    // neighbours: lower z-slab first, then upper -- the order of the ghost columns generated by
    // ramd_mat_gen_poisson7_slab ([lower plane | upper plane])
    std::vector<int> peers, soff(1, 0), roff(1, 0), bidx;
    if(z_begin > 0)
    {
        if(rank == 0)
            throw std::runtime_error("setup_poisson: rank 0 must own the first slab");
        peers.push_back(rank - 1);
        for(int64_t i = 0; i < N2; ++i)
            bidx.push_back((int)i); // my first plane goes down
        soff.push_back((int)bidx.size());
        roff.push_back(roff.back() + (int)N2);
    }
    if(z_end < N)
    {
        if(rank == np - 1)
            throw std::runtime_error("setup_poisson: the last rank must own the last slab");
        peers.push_back(rank + 1);
        for(int64_t i = 0; i < N2; ++i)
            bidx.push_back((int)(nloc - N2 + i)); // my last plane goes up
        soff.push_back((int)bidx.size());
        roff.push_back(roff.back() + (int)N2);
    }
    g->pm.SetGlobalNrow(n);
    g->pm.SetGlobalNcol(n);
    g->pm.SetLocalNrow(nloc);
    g->pm.SetLocalNcol(nloc);
    g->pm.SetBoundaryIndex((int)bidx.size(), bidx.data());
    g->pm.SetReceivers((int)peers.size(), peers.data(), roff.data());
    g->pm.SetSenders((int)peers.size(), peers.data(), soff.data());
    g->A.SetParallelManager(g->pm);
    if(lap27)
        g->A.GenerateLaplace27Slab(N, N, N, z_begin, z_end);
    else
        g->A.GeneratePoisson7Slab(N, lo, hi);
    g->A.CompactGhost();
    g->alloc_vectors();
    g->setup = true;
    GUARD_END
}

int ramd_gsolver_setup_csr(ramd_gsolver_t g, int64_t global_nrow, int local_nrow, int64_t int_nnz,
                           const int32_t* int_rp, const int32_t* int_ci, const double* int_val,
                           int64_t gh_nnz, const int32_t* gh_rp, const int32_t* gh_ci,
                           const double* gh_val, int npeers, const int* peers, const int* send_offset,
                           const int* recv_offset, const int* boundary_index)
{
    if(!g || local_nrow < 0 || !int_rp || !gh_rp || npeers < 0)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    g->pm.SetGlobalNrow(global_nrow);
    g->pm.SetGlobalNcol(global_nrow);
    g->pm.SetLocalNrow(local_nrow);
    g->pm.SetLocalNcol(local_nrow);
    const int nsend = npeers ? send_offset[npeers] : 0;
    g->pm.SetBoundaryIndex(nsend, boundary_index);
    const int zero[1] = {0};
    g->pm.SetReceivers(npeers, peers, npeers ? recv_offset : zero);
    g->pm.SetSenders(npeers, peers, npeers ? send_offset : zero);
    g->A.SetParallelManager(g->pm);
    auto dup = [](const auto* p, int64_t n) {
        typedef typename std::remove_cv<typename std::remove_pointer<decltype(p)>::type>::type X;
        X* q = new X[(size_t)std::max<int64_t>(n, 1)];
        std::copy(p, p + n, q);
        return q;
    };
    {
        PtrType* rp = dup(int_rp, (int64_t)local_nrow + 1);
        int*     ci = dup(int_ci, int_nnz);
        double*  va = dup(int_val, int_nnz);
        g->A.SetLocalDataPtrCSR(&rp, &ci, &va, "A", int_nnz);
    }
    {
        PtrType* rp = dup(gh_rp, (int64_t)local_nrow + 1);
        int*     ci = dup(gh_ci, gh_nnz);
        double*  va = dup(gh_val, gh_nnz);
        g->A.SetGhostDataPtrCSR(&rp, &ci, &va, "A", gh_nnz);
    }
    g->A.MoveToAccelerator();
    g->A.CompactGhost();
    g->alloc_vectors();
    g->setup = true;
    GUARD_END
}

int ramd_gsolver_convert(ramd_gsolver_t g, int format)
{
    if(!g || !g->setup)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    g->A.ConvertTo((unsigned)format);
    GUARD_END
}
int ramd_gsolver_init(ramd_gsolver_t g, double a, double r, double d, int mn, int mx)
{
    if(!g)
        return RAMD_ERR_ARG;
    g->ls()->Init(a, r, d, mn, mx);
    return RAMD_OK;
}
int ramd_gsolver_set_basis(ramd_gsolver_t g, int m)
{
    if(!g || m < 1)
        return RAMD_ERR_ARG;
    g->gmres.SetBasisSize(m);
    return RAMD_OK;
}
int ramd_gsolver_set_verbose(ramd_gsolver_t g, int v)
{
    if(!g)
        return RAMD_ERR_ARG;
    g->ls()->Verbose(v);
    return RAMD_OK;
}
// the local preconditioner under BlockJacobi takes the parameters / the format request of a stand-alone solver's
int ramd_gsolver_set_precond_params(ramd_gsolver_t g, double p0, double p1, double p2)
{
    if(!g || g->mixed || g->built || check_precond_params(g->pc_kind, p0, p1, p2) != RAMD_OK)
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    g->precs.set_params(g->pc_kind, p0, p1, p2);
    GUARD_END
}
int ramd_gsolver_set_precond_format(ramd_gsolver_t g, int format)
{
    if(!g || g->mixed || g->built
       || (g->pc_kind != RAMD_PC_TNS && g->pc_kind != RAMD_PC_MULTIELIM && g->pc_kind != RAMD_PC_MCSGS && g->pc_kind != RAMD_PC_MCGS
           && g->pc_kind != RAMD_PC_MCILU))
        return RAMD_ERR_ARG;
    GUARD_BEGIN
    g->precs.set_format(g->pc_kind, format);
    GUARD_END
}
int ramd_gsolver_build(ramd_gsolver_t g)
{
    if(!g || !g->setup)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    if(g->built)
        g->ls()->Clear();
    g->ls()->SetOperator(g->A);
    if(g->mixed)
    {
        if(g->pc_kind == RAMD_PC_JACOBI)
            g->inner()->SetPreconditioner(g->jacobif);
        g->mp.Set(*g->inner());
        g->mp.Build();
        g->built = true;
        return RAMD_OK;
    }
    if(g->pc_kind == RAMD_PC_JACOBI)
        g->ls()->SetPreconditioner(g->jacobi);
    else if(g->pc_kind == RAMD_PC_GLOBAL_UAAMG || g->pc_kind == RAMD_PC_GLOBAL_SAAMG)
    {
        g->guaamg.SetCoarseningStrategy(PMIS);
        g->gsaamg.SetCoarseningStrategy(PMIS);
        g->guaamg.Verbose(0);
        g->gsaamg.Verbose(0);
        if(g->pc_kind == RAMD_PC_GLOBAL_UAAMG)
            g->ls()->SetPreconditioner(g->guaamg);
        else
            g->ls()->SetPreconditioner(g->gsaamg);
    }
    else if(g->pc_kind != RAMD_PC_NONE) // BlockJacobi over ranks: the local preconditioner on the interior block
    {
        g->bj.Set(*g->precs.get(g->pc_kind));
        g->ls()->SetPreconditioner(g->bj);
    }
    g->ls()->Build();
    g->built = true;
    GUARD_END
}
int ramd_gsolver_amg_info(ramd_gsolver_t g, int* levels, int64_t* coarsest_rows, double* worst_galerkin_defect)
{
    if(!g || !g->built || (g->pc_kind != RAMD_PC_GLOBAL_UAAMG && g->pc_kind != RAMD_PC_GLOBAL_SAAMG))
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    BaseAMG<ramd_gsolver_s::GM, ramd_gsolver_s::GV, double>* amg
        = g->pc_kind == RAMD_PC_GLOBAL_UAAMG ? (BaseAMG<ramd_gsolver_s::GM, ramd_gsolver_s::GV, double>*)&g->guaamg : &g->gsaamg;
    const int L = amg->GetNumLevels();
    double    worst = 0.0;
    for(int l = 0; l + 1 < L; ++l)
    {
        ramd_gsolver_s::GV xc;
        xc.CloneBackend(*amg->GetLevelOperator(l + 1));
        xc.Allocate("probe", amg->GetLevelOperator(l + 1)->GetM());
        xc.GetInterior().SetRandomUniform(1234ull + 77ull * (unsigned)g->pm.GetRank() + (unsigned)l, -1.0, 1.0);
        worst = std::max(worst, (double)amg->GalerkinDefect(l, xc));
    }
    if(levels)
        *levels = L;
    if(coarsest_rows)
        *coarsest_rows = amg->GetLevelOperator(L - 1)->GetM();
    if(worst_galerkin_defect)
        *worst_galerkin_defect = worst;
    GUARD_END
}
int ramd_gsolver_amg_level(ramd_gsolver_t g, int level, int64_t* global_rows, int64_t* local_entries,
                           double* norm_of_row_sums)
{
    if(!g || !g->built || (g->pc_kind != RAMD_PC_GLOBAL_UAAMG && g->pc_kind != RAMD_PC_GLOBAL_SAAMG))
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    BaseAMG<ramd_gsolver_s::GM, ramd_gsolver_s::GV, double>* amg
        = g->pc_kind == RAMD_PC_GLOBAL_UAAMG ? (BaseAMG<ramd_gsolver_s::GM, ramd_gsolver_s::GV, double>*)&g->guaamg : &g->gsaamg;
    if(level < 0 || level >= amg->GetNumLevels())
        return RAMD_ERR_ARG;
    const ramd_gsolver_s::GM* A = amg->GetLevelOperator(level);
    ramd_gsolver_s::GV        one, y;
    one.CloneBackend(*A);
    y.CloneBackend(*A);
    one.Allocate("ones", A->GetM());
    y.Allocate("row sums", A->GetM());
    one.Ones();
    A->Apply(one, &y);
    if(global_rows)
        *global_rows = A->GetM();
    if(local_entries)
        *local_entries = A->GetLocalNnz() + A->GetGhostNnz();
    if(norm_of_row_sums)
        *norm_of_row_sums = y.Norm();
    GUARD_END
}
int ramd_gsolver_apply(ramd_gsolver_t g, const double* x_local, double* y_local)
{
    if(!g || !g->setup || !x_local || !y_local)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    g->x.GetInterior().CopyFromHostData(x_local);
    g->A.Apply(g->x, &g->tmp);
    g->tmp.GetInterior().CopyToHostData(y_local);
    GUARD_END
}
int ramd_gsolver_precond_apply(ramd_gsolver_t g, const double* rhs_local, double* x_local)
{
    if(!g || !g->built || g->mixed || g->pc_kind == RAMD_PC_NONE || !rhs_local || !x_local)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    Solver<ramd_gsolver_s::GM, ramd_gsolver_s::GV, double>* p = &g->bj;
    if(g->pc_kind == RAMD_PC_JACOBI)
        p = &g->jacobi;
    else if(g->pc_kind == RAMD_PC_GLOBAL_UAAMG)
        p = &g->guaamg;
    else if(g->pc_kind == RAMD_PC_GLOBAL_SAAMG)
        p = &g->gsaamg;
    g->rhs.GetInterior().CopyFromHostData(rhs_local);
    p->SolveZeroSol(g->rhs, &g->tmp);
    g->tmp.GetInterior().CopyToHostData(x_local);
    GUARD_END
}
int ramd_gsolver_solve(ramd_gsolver_t g, const double* rhs_local, double* x_local)
{
    if(!g || !g->built || !x_local)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    if(rhs_local)
        g->rhs.GetInterior().CopyFromHostData(rhs_local);
    else
    {
        g->tmp.Ones();
        g->A.Apply(g->tmp, &g->rhs);
    }
    g->x.GetInterior().CopyFromHostData(x_local);
    g->ls()->Solve(g->rhs, &g->x);
    g->x.GetInterior().CopyToHostData(x_local);
    GUARD_END
}
int ramd_gsolver_solve_ones(ramd_gsolver_t g)
{
    if(!g || !g->built)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    g->tmp.Ones();
    g->A.Apply(g->tmp, &g->rhs);
    g->x.Zeros();
    g->ls()->Solve(g->rhs, &g->x);
    GUARD_END
}
int ramd_gsolver_prepare_ones(ramd_gsolver_t g)
{
    if(!g || !g->setup)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    g->tmp.Ones();
    g->A.Apply(g->tmp, &g->rhs);
    g->x.Zeros();
    GUARD_END
}
int ramd_gsolver_solve_device(ramd_gsolver_t g)
{
    if(!g || !g->built)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    g->ls()->Solve(g->rhs, &g->x);
    GUARD_END
}
int ramd_gsolver_set_time_mark(ramd_gsolver_t g, int iteration)
{
    if(!g)
        return RAMD_ERR_ARG;
    g->ls()->SetTimeMark(iteration);
    return RAMD_OK;
}
int ramd_gsolver_seconds_since_time_mark(ramd_gsolver_t g, double* seconds)
{
    if(!g || !seconds)
        return RAMD_ERR_ARG;
    *seconds = g->ls()->GetSecondsSinceTimeMark();
    return RAMD_OK;
}
int ramd_gsolver_result(ramd_gsolver_t g, int* iters, int* status, double* final_res)
{
    if(!g)
        return RAMD_ERR_ARG;
    if(iters)
        *iters = g->ls()->GetIterationCount();
    if(status)
        *status = g->ls()->GetSolverStatus();
    if(final_res)
        *final_res = g->ls()->GetCurrentResidual();
    return RAMD_OK;
}
int ramd_gsolver_dot_check(ramd_gsolver_t g, double* xx)
{
    if(!g || !g->setup || !xx)
        return RAMD_ERR_STATE;
    GUARD_BEGIN
    *xx = g->x.Dot(g->x);
    GUARD_END
}

} // extern "C"
