// Chebyshev<GlobalMatrix, GlobalVector> on several ranks of a row-block split that share ONE device, next to the LocalMatrix run.
//   global_chebyshev_driver <ranks> <N> <none|jacobi> <lambda_min> <lambda_max> <max_iter> <outfile>
// ranks = 0: the LocalMatrix / LocalVector run.  ranks >= 1: that many processes (forked before anything touches the device),
// each with the piece distribute_matrix gives it of the 7-point Poisson operator on N^3, halo and scalar sums through the
// callback transport.  The callbacks are a few lines over a block of shared memory: one mailbox per ordered pair of ranks
// for the halo segments, one table of partial sums that every rank adds in rank order (so all ranks see the same sum).
// The parent never opens the device; it collects the ranks' pieces and writes
//   "<iters> <status> <history entries> <solution entries>" and then the history and the solution, one %.17g per line.
#include <rocalution/rocalution.hpp>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include <sched.h>
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

using namespace rocalution;

namespace
{
constexpr int    kMaxRanks   = 4;
constexpr size_t kBoxBytes   = 1 << 20; // a halo segment of N^3 <= 64^3: one plane of doubles and more
constexpr int    kMaxScalars = 512;
constexpr int    kMaxHist    = 4096;
constexpr double kWaitSeconds = 30.0; // (a rank that died must not leave the others waiting, with the device open)

struct Mailbox
{
    std::atomic<long> written, taken;
    char              data[kBoxBytes];
};
struct Shared
{
    Mailbox           box[kMaxRanks][kMaxRanks]; // [from][to]
    std::atomic<long> arrived, round;
    double            part[kMaxRanks][kMaxScalars];
    // results
    int    iters[kMaxRanks], status[kMaxRanks], nhist[kMaxRanks];
    double hist[kMaxRanks][kMaxHist];
};
struct Rank
{
    Shared* sh;
    int     rank, size;
};

bool wait_until(const std::atomic<long>& a, long at_least)
{
    const auto t0 = std::chrono::steady_clock::now();
    for(long spins = 0; a.load(std::memory_order_acquire) < at_least; ++spins)
    {
        if((spins & 1023) == 1023 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kWaitSeconds)
            return false;
        sched_yield();
    }
    return true;
}
bool barrier(Rank* r)
{
    const long round = r->sh->round.load(std::memory_order_acquire);
    if(r->sh->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == (long)r->size * (round + 1))
        r->sh->round.store(round + 1, std::memory_order_release);
    return wait_until(r->sh->round, round + 1);
}
int cb_exchange(void* user, int npeers, const int* peers, const void* send, const int64_t* so, void* recv, const int64_t* ro)
{
    Rank* r = (Rank*)user;
    for(int k = 0; k < npeers; ++k)
    {
        Mailbox&     m = r->sh->box[r->rank][peers[k]];
        const size_t n = (size_t)(so[k + 1] - so[k]);
        if(n > kBoxBytes || !wait_until(m.taken, m.written.load(std::memory_order_acquire)))
            return 1;
        std::memcpy(m.data, (const char*)send + so[k], n);
        m.written.fetch_add(1, std::memory_order_release);
    }
    for(int k = 0; k < npeers; ++k)
    {
        Mailbox&     m = r->sh->box[peers[k]][r->rank];
        const size_t n = (size_t)(ro[k + 1] - ro[k]);
        if(n > kBoxBytes || !wait_until(m.written, m.taken.load(std::memory_order_acquire) + 1))
            return 1;
        std::memcpy((char*)recv + ro[k], m.data, n);
        m.taken.fetch_add(1, std::memory_order_release);
    }
    return 0;
}
int cb_allreduce(void* user, double* values, int count)
{
    Rank* r = (Rank*)user;
    if(count > kMaxScalars)
        return 1;
    std::memcpy(r->sh->part[r->rank], values, sizeof(double) * (size_t)count);
    if(!barrier(r))
        return 1;
    for(int k = 0; k < count; ++k)
    {
        double s = 0.0;
        for(int q = 0; q < r->size; ++q)
            s += r->sh->part[q][k];
        values[k] = s;
    }
    return barrier(r) ? 0 : 1; // (nobody overwrites its partial sums before everybody has read them)
}

void poisson7(int N, std::vector<PtrType>& rp, std::vector<int>& col, std::vector<double>& val)
{
    rp.assign(1, 0);
    for(int k = 0; k < N; ++k)
        for(int j = 0; j < N; ++j)
            for(int i = 0; i < N; ++i)
            {
                const int r = (k * N + j) * N + i;
                if(k > 0) { col.push_back(r - N * N); val.push_back(-1); }
                if(j > 0) { col.push_back(r - N); val.push_back(-1); }
                if(i > 0) { col.push_back(r - 1); val.push_back(-1); }
                col.push_back(r); val.push_back(6);
                if(i < N - 1) { col.push_back(r + 1); val.push_back(-1); }
                if(j < N - 1) { col.push_back(r + N); val.push_back(-1); }
                if(k < N - 1) { col.push_back(r + N * N); val.push_back(-1); }
                rp.push_back((PtrType)col.size());
            }
}

struct Args
{
    int    N, max_iter;
    bool   jacobi;
    double lo, hi;
};

template <class Mat, class Vec>
void solve(const Args& a, Mat& A, Vec& rhs, Vec& x, Shared* sh, int slot)
{
    Chebyshev<Mat, Vec, double> ls;
    Jacobi<Mat, Vec, double>    jac;
    ls.Set(a.lo, a.hi);
    ls.InitMaxIter(a.max_iter);
    ls.RecordResidualHistory();
    ls.Verbose(0);
    ls.SetOperator(A);
    if(a.jacobi)
        ls.SetPreconditioner(jac);
    ls.Build();
    ls.Solve(rhs, &x);
    sh->iters[slot]  = ls.GetIterationCount();
    sh->status[slot] = ls.GetSolverStatus();
    const std::vector<double>& h = ls.GetResidualHistory();
    sh->nhist[slot] = (int)h.size() < kMaxHist ? (int)h.size() : kMaxHist;
    std::copy(h.begin(), h.begin() + sh->nhist[slot], sh->hist[slot]);
    ls.Clear();
}

// one rank (size >= 1) or the Local run (size == 0); its part of x goes to xout[first ...)
int run_rank(const Args& a, Shared* sh, int rank, int size, double* xout)
{
    init_rocalution();
    std::vector<PtrType> rp;
    std::vector<int>     col;
    std::vector<double>  val;
    poisson7(a.N, rp, col, val);
    const int64_t n = (int64_t)rp.size() - 1, nnz = (int64_t)col.size();
    LocalMatrix<double> lmat;
    lmat.AllocateCSR("A", nnz, n, n);
    lmat.CopyFromCSR(rp.data(), col.data(), val.data());
    if(size == 0)
    {
        LocalVector<double> x, rhs, e;
        x.Allocate("x", n); rhs.Allocate("rhs", n); e.Allocate("e", n);
        lmat.MoveToAccelerator(); x.MoveToAccelerator(); rhs.MoveToAccelerator(); e.MoveToAccelerator();
        e.Ones(); lmat.Apply(e, &rhs); x.Zeros();
        solve(a, lmat, rhs, x, sh, 0);
        x.CopyToData(xout);
    }
    else
    {
        Rank       me = {sh, rank, size};
        ramd_comm_t comm = NULL;
        if(ramd_comm_init_callback(rank, size, cb_exchange, cb_allreduce, &me, &comm) != RAMD_OK)
            return 1;
        {
            ParallelManager      pm;
            GlobalMatrix<double> gmat;
            distribute_matrix(comm, &lmat, &gmat, &pm);
            gmat.MoveToAccelerator();
            GlobalVector<double> x(pm), rhs(pm), e(pm);
            x.Allocate("x", n); rhs.Allocate("rhs", n); e.Allocate("e", n);
            x.MoveToAccelerator(); rhs.MoveToAccelerator(); e.MoveToAccelerator();
            e.Ones(); gmat.Apply(e, &rhs); x.Zeros();
            solve(a, gmat, rhs, x, sh, rank);
            x.GetInterior().CopyToData(xout + row_block_offsets(n, size)[(size_t)rank]);
        }
        if(ramd_comm_destroy(comm) != RAMD_OK)
            return 1;
    }
    stop_rocalution();
    return 0;
}
} // namespace

int main(int argc, char** argv)
{
    if(argc < 8)
    {
        std::fprintf(stderr, "%s <ranks> <N> <none|jacobi> <lambda_min> <lambda_max> <max_iter> <outfile>\n", argv[0]);
        return 2;
    }
    const int size = std::atoi(argv[1]);
    Args      a;
    a.N        = std::atoi(argv[2]);
    a.jacobi   = std::string(argv[3]) == "jacobi";
    a.lo       = std::atof(argv[4]);
    a.hi       = std::atof(argv[5]);
    a.max_iter = std::atoi(argv[6]);
    if(size < 0 || size > kMaxRanks || a.N < 2 || a.N > 64 || a.max_iter < 1 || a.max_iter >= kMaxHist)
        return 2;
    const size_t n = (size_t)a.N * a.N * a.N;
    void* mem = mmap(NULL, sizeof(Shared) + sizeof(double) * n, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if(mem == MAP_FAILED)
        return 3;
    Shared* sh   = new(mem) Shared; // (anonymous shared pages start zeroed; the atomics of Shared are lock-free longs)
    double* xout = (double*)((char*)mem + sizeof(Shared));
    const int          procs = size == 0 ? 1 : size;
    std::vector<pid_t> kids;
    for(int r = 0; r < procs; ++r)
    {
        const pid_t p = fork();
        if(p < 0)
            return 3;
        if(p == 0)
            _exit(run_rank(a, sh, r, size, xout));
        kids.push_back(p);
    }
    int bad = 0;
    for(pid_t p : kids)
    {
        int st = 0;
        if(waitpid(p, &st, 0) != p || !WIFEXITED(st) || WEXITSTATUS(st) != 0)
            ++bad;
    }
    if(bad)
    {
        std::printf("global_chebyshev_driver: %d rank(s) failed\n", bad);
        return 1;
    }
    for(int r = 1; r < procs; ++r) // every rank has seen the same all-reduced norms and taken the same decisions
        if(sh->iters[r] != sh->iters[0] || sh->status[r] != sh->status[0] || sh->nhist[r] != sh->nhist[0]
           || std::memcmp(sh->hist[r], sh->hist[0], sizeof(double) * (size_t)sh->nhist[0]) != 0)
        {
            std::printf("global_chebyshev_driver: rank %d disagrees with rank 0\n", r);
            return 1;
        }
    FILE* f = std::fopen(argv[7], "w");
    if(!f)
        return 3;
    std::fprintf(f, "%d %d %d %zu\n", sh->iters[0], sh->status[0], sh->nhist[0], n);
    for(int k = 0; k < sh->nhist[0]; ++k)
        std::fprintf(f, "%.17g\n", sh->hist[0][k]);
    for(size_t i = 0; i < n; ++i)
        std::fprintf(f, "%.17g\n", xout[i]);
    std::fclose(f);
    std::printf("global_chebyshev_driver ok: %d rank(s), %d iterations, status %d\n", size, sh->iters[0], sh->status[0]);
    return 0;
}
