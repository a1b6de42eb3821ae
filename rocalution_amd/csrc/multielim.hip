// multielim.hip -- the MultiElimination preconditioner (multi-elimination ILU) on gfx950, one elimination level per plan.
//
// Reference: src/solvers/preconditioners/preconditioner_multielimination.cpp (Build :174-309, Solve :312-342);
// LocalMatrix::MaximalIndependentSet (host_matrix_csr.cpp:2602-2663, the same host sweep in hip_matrix_csr.cpp:3833-3912) and
// LocalMatrix::Compress (host_matrix_csr.cpp:3679-3740).
//
// With the permutation p of the independent set (members first) P A P^T = [D F; E C], D diagonal, and
//     AA = C - (E D^-1) F          (the Schur complement, optionally compressed)
// the apply is  rhs_ = P rhs ; x1 = rhs_[0:size] ; rhs2 = rhs_[size:] ; rhs2 += (-1) E x1 ; x2 = AA^-1 rhs2 (the caller's
// solver) ; x1 += (-1) F x2 ; x1 *= inv_D ; x = P^T [x1; x2], E standing for E D^-1.  A plan holds E, F, inv_D, p and AA and
// applies the two halves around the caller's solve in one of two forms that give the same bits:
//   stepwise (form 0)  the reference's steps, one library call each (three copies, ApplyAdd | ApplyAdd, PointWiseMult, two
//                      copies, a permuted copy); E and F in any format
//   fused    (form 1)  k_me_down and k_me_up: the permutation is folded into E's column indices at Build() (columns in the
//                      operator's own numbering) and into the row gathers through q = p^-1; no intermediate vector exists
// Arithmetic is ApplyAdd's (host_matrix_csr.cpp:737-769): out += (scalar * val) * in, entry by entry in row order.
#include "csr_filter.hpp"
#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <string>
#include <vector>

namespace ramd
{

constexpr int kMeDefaultRounds = 4096; // rounds of the fixed point before the host sweep takes over (max_rounds = 0)
constexpr int kMeGW            = 4; // entries of a row in flight per lane

// what form = -1 (auto) takes: the stepwise form, by measurement (profiles/multielim.md: E and F of a stencil operator run
// the value-pattern product, which reads neither columns nor values, and the copies are contiguous; the fused kernels walk
// the stored rows a thread each and gather through q: 0.62 ms against 0.36 ms at 256^3)
constexpr bool kMeAutoFused = false;

enum
{
    ME_UNDECIDED = 0,
    ME_IN        = 1,
    ME_OUT       = -1
};

// One round of the fixed point that reaches the sequential sweep's set on a structurally symmetric pattern: a row is out
// once a lower-numbered neighbour has joined and joins once every lower-numbered neighbour is out.  A decision is final
// and does not depend on the order in which rows are looked at, so the state is updated in place: a row may see a
// decision of this very round.  *left counts the rows this round leaves undecided.
__global__ __launch_bounds__(kBlock) void k_mis_round(int nrow, const int* __restrict__ rp, const int* __restrict__ ci, int* state,
                                                      int* __restrict__ left)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    int           und = 0;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        if(state[i] != ME_UNDECIDED)
            continue;
        bool out = false, wait = false;
        for(int j = rp[i]; j < rp[i + 1]; ++j)
        {
            const int c = ci[j];
            if(c >= (int)i || c < 0)
                continue;
            const int s = state[c];
            out         = out || s == ME_IN;
            wait        = wait || s == ME_UNDECIDED;
        }
        if(out)
            state[i] = ME_OUT;
        else if(!wait)
            state[i] = ME_IN;
        else
            ++und;
    }
    if(und)
        atomicAdd(left, und);
}

__global__ __launch_bounds__(kBlock) void k_mis_flags(int nrow, const int* __restrict__ state, int* __restrict__ flag)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nrow; i += gsz)
        flag[i] = (i < nrow && state[i] == ME_IN) ? 1 : 0;
}

// members first, in order, then the rest, in order (host_matrix_csr.cpp:2639-2651); pos = exclusive scan of the flags
__global__ __launch_bounds__(kBlock) void k_mis_perm(int nrow, const int* __restrict__ state, const int* __restrict__ pos,
                                                     int* __restrict__ perm)
{
    const int64_t gsz  = (int64_t)gridDim.x * blockDim.x;
    const int     size = pos[nrow];
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
        perm[i] = state[i] == ME_IN ? pos[i] : size + (int)i - pos[i];
}

// *bad = 1 where a row's columns are not strictly ascending
__global__ __launch_bounds__(kBlock) void k_me_rows_unsorted(int nrow, const int* __restrict__ rp, const int* __restrict__ ci,
                                                             int* __restrict__ bad)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    bool          d   = false;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
        for(int j = rp[i] + 1; j < rp[i + 1]; ++j)
            d = d || ci[j - 1] >= ci[j];
    if(d)
        *bad = 1;
}

// q[p[i]] = i ; out[j] = q[in[j]]
__global__ __launch_bounds__(kBlock) void k_me_invert(int n, const int* __restrict__ p, int* __restrict__ q)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
        q[p[i]] = (int)i;
}
__global__ __launch_bounds__(kBlock) void k_me_map(int64_t n, const int* __restrict__ in, const int* __restrict__ q,
                                                   int* __restrict__ out)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
        out[i] = q[in[i]];
}

// Compress: an entry stays if |val| > drop (compared in double) or it is on the diagonal
struct CompressRule // (csr_filter.hpp)
{
    static constexpr bool kRowsOnce = true;
    double                drop;
    __device__ FilterRow row(int64_t i) const { return FilterRow{(int)i}; }
    template <typename T>
    __device__ bool keep(const FilterRow& r, int col, T v) const { return fabs((double)v) > drop || col == r.src; }
    __device__ int  col(const FilterRow&, int col) const { return col; }
};

// acc += ((-1) * a_j) * v[c_j] over a row's entries in storage order, kMeGW entries in flight; no load under a branch: a
// lane past its row's end reads entry 0 / element 0 and keeps its sum by a select
template <typename T>
__device__ __forceinline__ T me_row_sub(T acc, int b, int e, const int* __restrict__ ci, const T* __restrict__ val,
                                        const T* __restrict__ v)
{
    for(int jb = b; __ballot(jb < e) != 0ull; jb += kMeGW)
    {
        T    a[kMeGW], xv[kMeGW];
        int  c[kMeGW];
        bool ok[kMeGW];
#pragma unroll
        for(int k = 0; k < kMeGW; ++k)
        {
            ok[k]       = jb + k < e;
            const int j = ok[k] ? jb + k : 0;
            a[k]        = val[j];
            c[k]        = ok[k] ? ci[j] : 0;
        }
#pragma unroll
        for(int k = 0; k < kMeGW; ++k)
            xv[k] = v[c[k]];
#pragma unroll
        for(int k = 0; k < kMeGW; ++k)
        {
            const T s2 = acc + ((T)(-1) * a[k]) * xv[k];
            acc        = ok[k] ? s2 : acc;
        }
    }
    return acc;
}

// rhs2[i] = rhs[q[size + i]] + sum_j ((-1) * E_ij) * rhs[col'_j]   (col' = E's columns in the operator's numbering)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_me_down(int m2, int size, const int* __restrict__ rp, const int* __restrict__ ci,
                                                    const T* __restrict__ val, const int* __restrict__ q,
                                                    const T* __restrict__ rhs, T* __restrict__ rhs2)
{
    const int  i    = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < m2;
    int        b = 0, e = 0;
    T          acc = (T)0;
    if(live)
    {
        b   = rp[i];
        e   = rp[i + 1];
        acc = rhs[q[size + i]];
    }
    acc = me_row_sub<T>(acc, b, e, ci, val, rhs);
    if(live)
        rhs2[i] = acc;
}

// i < size : x[q[i]] = (rhs[q[i]] + sum_j ((-1) * F_ij) * x2[col_j]) * inv_D[i]     i >= size : x[q[i]] = x2[i - size]
template <typename T>
__global__ __launch_bounds__(kBlock) void k_me_up(int n, int size, const int* __restrict__ rp, const int* __restrict__ ci,
                                                  const T* __restrict__ val, const int* __restrict__ q,
                                                  const T* __restrict__ dinv, const T* __restrict__ rhs,
                                                  const T* __restrict__ x2, T* __restrict__ x)
{
    const int  i    = blockIdx.x * kBlock + threadIdx.x;
    const bool top  = i < size;
    int        b = 0, e = 0, qi = 0;
    T          acc = (T)0;
    if(i < n)
        qi = q[i];
    if(top)
    {
        b   = rp ? rp[i] : 0;
        e   = rp ? rp[i + 1] : 0;
        acc = rhs[qi];
    }
    if(rp) // (wave-uniform: F has no entry at all)
        acc = me_row_sub<T>(acc, b, e, ci, val, x2);
    if(top)
        x[qi] = acc * dinv[i];
    else if(i < n)
        x[qi] = x2[i - size];
}

} // namespace ramd

using namespace ramd;

struct ramd_me_s
{
    int     dtype = RAMD_F64;
    int     n = 0, size = 0;
    int     form     = 1; // 0 stepwise, 1 fused
    int     mis_path = 0, mis_rounds = 0, mis_sym = 0;
    int64_t aa_nnz = 0;
    ramd_vec_t perm = nullptr, dinv = nullptr;
    ramd_mat_t E = nullptr, F = nullptr, AA = nullptr;
    int*       q     = nullptr; // [n] inverse permutation
    int*       e_col = nullptr; // [nnz(E)] fused form: E's columns in the operator's numbering
    // stepwise form: the reference's work vectors
    ramd_vec_t rhs_ = nullptr, x_ = nullptr, x1 = nullptr;
    const ramd_vec_s* down_rhs = nullptr; // the rhs whose down left x1 behind; up continues that one and no other
    void       release()
    {
        dev_free(&q);
        dev_free(&e_col);
        ramd_mat_t* ms[] = {&E, &F, &AA};
        for(ramd_mat_t* m : ms)
        {
            if(*m)
                (void)ramd_mat_destroy(*m);
            *m = nullptr;
        }
        ramd_vec_t* vs[] = {&perm, &dinv, &rhs_, &x_, &x1};
        for(ramd_vec_t* v : vs)
        {
            if(*v)
                (void)ramd_vec_destroy(*v);
            *v = nullptr;
        }
    }
};

namespace
{

int me_new_vec(int dtype, int64_t n, ramd_vec_t* out)
{
    RAMD_TRY(ramd_vec_create(dtype, out));
    return n > 0 ? ramd_vec_allocate(*out, n) : RAMD_OK;
}

// is the pattern structurally symmetric?  Rows strictly ascending and the offsets and columns of A^T equal to A's; a
// symmetric pattern with unsorted rows is reported as not symmetric (the host sweep then gives the same set)
int mis_symmetric(const ramd_mat_s* A, bool* sym)
{
    Backend& b = backend();
    *sym       = false;
    if(A->nnz <= 0)
    {
        *sym = true;
        return RAMD_OK;
    }
    int* bad = nullptr;
    int  hb  = 0;
    RAMD_TRY(dev_alloc(&bad, 1));
    int s = hipMemsetAsync(bad, 0, sizeof(int), b.cur) == hipSuccess ? RAMD_OK : RAMD_ERR_HIP;
    if(s == RAMD_OK)
    {
        hipLaunchKernelGGL(k_me_rows_unsorted, dim3(ew_grid(A->nrow)), dim3(kBlock), 0, b.cur, A->nrow, A->rp, A->ci, bad);
        if(hipGetLastError() != hipSuccess || hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
           || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    ramd_mat_t t = nullptr;
    if(s == RAMD_OK && !hb)
    {
        s = ramd_mat_create(A->dtype, &t);
        if(s == RAMD_OK)
            s = mat_transpose(A, t);
        if(s == RAMD_OK && t->nnz != A->nnz)
            hb = 1;
        else if(s == RAMD_OK)
        {
            dev_words_differ(A->rp, t->rp, (int64_t)A->nrow + 1, bad);
            dev_words_differ(A->ci, t->ci, A->nnz, bad);
            if(hipGetLastError() != hipSuccess || hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess)
                s = RAMD_ERR_HIP;
        }
    }
    if(t)
        (void)ramd_mat_destroy(t);
    dev_free(&bad);
    if(s != RAMD_OK)
        RAMD_FAIL(s, "MaximalIndependentSet: examining the pattern failed");
    *sym = hb == 0;
    return RAMD_OK;
}

// the fixed point on the device; *done = false when the rounds ran out
int mis_device(const ramd_mat_s* A, int max_rounds, ramd_vec_s* perm, int* size, int* rounds, bool* done)
{
    Backend&  b = backend();
    const int n = A->nrow;
    *done       = false;
    *rounds     = 0;
    int *state = nullptr, *left = nullptr, *pos = nullptr;
    RAMD_TRY(dev_alloc(&state, n));
    int s = dev_alloc(&left, 1);
    if(s == RAMD_OK && hipMemsetAsync(state, 0, sizeof(int) * (size_t)n, b.cur) != hipSuccess)
        s = RAMD_ERR_HIP;
    int hl = 1;
    while(s == RAMD_OK && hl > 0 && *rounds < max_rounds)
    {
        if(hipMemsetAsync(left, 0, sizeof(int), b.cur) != hipSuccess)
        {
            s = RAMD_ERR_HIP;
            break;
        }
        hipLaunchKernelGGL(k_mis_round, dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, A->rp, A->ci, state, left);
        if((hipGetLastError() != hipSuccess || hipMemcpyAsync(&hl, left, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess))
            s = RAMD_ERR_HIP;
        ++*rounds;
    }
    if(s == RAMD_OK && hl == 0)
    {
        s = dev_alloc(&pos, (int64_t)n + 1);
        if(s == RAMD_OK)
        {
            hipLaunchKernelGGL(k_mis_flags, dim3(ew_grid((int64_t)n + 1)), dim3(kBlock), 0, b.cur, n, state, pos);
            s = device_exclusive_scan(pos, pos, (int64_t)n + 1);
        }
        if(s == RAMD_OK)
            s = ramd_vec_allocate(perm, n);
        if(s == RAMD_OK)
        {
            hipLaunchKernelGGL(k_mis_perm, dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, state, pos, (int*)perm->d);
            if(hipGetLastError() != hipSuccess || hipMemcpyAsync(size, pos + n, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess)
                s = RAMD_ERR_HIP;
        }
        *done = s == RAMD_OK;
    }
    dev_free(&state);
    dev_free(&left);
    dev_free(&pos);
    if(s != RAMD_OK)
        RAMD_FAIL(s, "MaximalIndependentSet: the device sweep failed");
    return RAMD_OK;
}

// the reference's sequential sweep on a host copy of the pattern (host_matrix_csr.cpp:2617-2651), from row 0: what the device
// rounds decided is not carried over (the result is the same, and the sweep is one pass).  *members counts the rows
// that are still in the set at the end -- fewer than *size when the sweep marked a row that had already joined
int mis_host(const ramd_mat_s* A, ramd_vec_s* perm, int* size, int* members)
{
    Backend&         b = backend();
    const int        n = A->nrow;
    std::vector<int> rp((size_t)n + 1), ci((size_t)(A->nnz > 0 ? A->nnz : 0));
    RAMD_HIP(hipMemcpyAsync(rp.data(), A->rp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, b.cur));
    if(A->nnz > 0)
        RAMD_HIP(hipMemcpyAsync(ci.data(), A->ci, sizeof(int) * (size_t)A->nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));
    std::vector<int> mis((size_t)n, 0), hp((size_t)n);
    int              sz = 0;
    for(int i = 0; i < n; ++i)
    {
        if(mis[i] != 0)
            continue;
        mis[i] = 1;
        ++sz;
        for(int j = rp[i]; j < rp[i + 1]; ++j)
        {
            const int c = ci[j];
            if(c != i && c >= 0 && c < n)
                mis[c] = -1;
        }
    }
    int pos = 0;
    for(int i = 0; i < n; ++i)
        if(mis[i] == 1)
            hp[i] = pos++;
        else
            hp[i] = sz + i - pos;
    *size    = sz;
    *members = pos;
    if(pos != sz) // not a permutation: nothing is handed out
        return RAMD_OK;
    RAMD_TRY(ramd_vec_allocate(perm, n));
    if(n > 0)
        RAMD_TRY(ramd_vec_copy_from_host(perm, hp.data()));
    return RAMD_OK;
}

int mis_impl(const ramd_mat_s* A, ramd_vec_s* perm, int max_rounds, int* size, int64_t* info)
{
    const int limit = max_rounds > 0 ? max_rounds : kMeDefaultRounds;
    bool      sym = false, done = false;
    int       rounds = 0, members = 0;
    RAMD_TRY(mis_symmetric(A, &sym));
    if(sym)
        RAMD_TRY(mis_device(A, limit, perm, size, &rounds, &done));
    if(done)
        members = *size;
    else
        RAMD_TRY(mis_host(A, perm, size, &members));
    if(info)
    {
        info[0] = done ? 0 : 1; // 0 device, 1 host finish
        info[1] = rounds;
        info[2] = sym ? 1 : 0;
        info[3] = members;
    }
    if(members != *size)
        RAMD_FAIL(RAMD_ERR_REFUSED,
                  "MaximalIndependentSet: the pattern is not structurally symmetric and the reference's sweep yields no permutation "
                  "here (it marked "
                      + std::to_string(*size - members) + " of its " + std::to_string(*size) + " members as removed afterwards)");
    return RAMD_OK;
}

// the kept entries go to a matrix of their own, whose arrays then replace m's: a failure leaves m as it was
int compress(ramd_mat_s* m, double drop)
{
    ramd_mat_s kept;
    kept.dtype  = m->dtype;
    const int s = csr_filter("Compress", "the result", CompressRule{drop}, m, m->rp, m->nrow, m->ncol, &kept);
    if(s != RAMD_OK)
    {
        mat_free_csr(&kept);
        RAMD_FAIL(s, "Compress failed");
    }
    mat_free_csr(m);
    mat_free_analysis(m);
    m->rp  = kept.rp;
    m->ci  = kept.ci;
    m->val = kept.val;
    m->nnz = kept.nnz;
    return RAMD_OK;
}

// Build() steps 1-9 with the library's own primitives (preconditioner_multielimination.cpp:204-247)
int me_build_steps(ramd_me_s* h, ramd_mat_t A, double drop, int max_rounds)
{
    Backend&   b = backend();
    const int  n = h->n;
    int64_t    info[4] = {0, 0, 0, 0};
    RAMD_TRY(ramd_vec_create(RAMD_I32, &h->perm));
    RAMD_TRY(mis_impl(A, h->perm, max_rounds, &h->size, info));
    h->mis_path   = (int)info[0];
    h->mis_rounds = (int)info[1];
    h->mis_sym    = (int)info[2];
    const int size = h->size, m2 = n - size;
    RAMD_TRY(ramd_mat_permute(A, h->perm));
    RAMD_TRY(dev_alloc(&h->q, n));
    hipLaunchKernelGGL(k_me_invert, dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, (const int*)h->perm->d, h->q);
    RAMD_HIP(hipGetLastError());
    ramd_mat_t D = nullptr, C = nullptr;
    int        s = ramd_mat_create(h->dtype, &D);
    if(s == RAMD_OK)
        s = ramd_mat_create(h->dtype, &h->AA);
    if(s == RAMD_OK)
        s = ramd_mat_extract_submatrix(A, 0, 0, size, size, D);
    if(s == RAMD_OK)
        s = ramd_vec_create(h->dtype, &h->dinv);
    if(s == RAMD_OK)
        s = ramd_mat_extract_inv_diag(D, h->dinv);
    if(D)
        (void)ramd_mat_destroy(D);
    RAMD_TRY(s);
    if(h->dinv->n != size)
        RAMD_FAIL(RAMD_ERR_ARG, "me_build: the rows of the independent set have no stored diagonal entry");
    if(m2 == 0) // every row is in the set (a diagonal operator): no E, F or last block
        return mat_alloc_csr(h->AA, 0, 0, 0);
    RAMD_TRY(ramd_mat_create(h->dtype, &h->F));
    RAMD_TRY(ramd_mat_create(h->dtype, &h->E));
    RAMD_TRY(ramd_mat_extract_submatrix(A, 0, size, size, m2, h->F));
    RAMD_TRY(ramd_mat_extract_submatrix(A, size, 0, m2, size, h->E));
    RAMD_TRY(ramd_mat_create(h->dtype, &C));
    s = ramd_mat_extract_submatrix(A, size, size, m2, m2, C);
    if(s == RAMD_OK && h->E->nnz > 0)
        s = ramd_mat_diag_mult(h->E, h->dinv, 0); // E = E D^-1
    if(s == RAMD_OK && h->E->nnz > 0 && h->F->nnz > 0)
    {
        s = ramd_mat_mat_mult(h->AA, h->E, h->F);
        if(s == RAMD_OK)
            s = ramd_mat_matrix_add(h->AA, C, -1.0, 1.0, 1); // AA = C - E D^-1 F
    }
    else if(s == RAMD_OK) // (no coupling between the set and the rest: the product has no entry, AA = C)
    {
        (void)ramd_mat_destroy(h->AA);
        h->AA = C;
        C     = nullptr;
    }
    if(C)
        (void)ramd_mat_destroy(C);
    RAMD_TRY(s);
    if(drop > 0.0 && h->AA->nnz > 0)
        RAMD_TRY(compress(h->AA, drop));
    h->aa_nnz = h->AA->nnz;
    return RAMD_OK;
}

template <typename T>
int me_down_t(ramd_me_s* h, ramd_vec_t rhs, ramd_vec_t rhs2)
{
    const int m2 = h->n - h->size;
    if(h->form == 1)
    {
        if(m2 == 0)
            return RAMD_OK;
        const ramd_mat_s* E = h->E;
        hipLaunchKernelGGL((k_me_down<T>), dim3((m2 + kBlock - 1) / kBlock), dim3(kBlock), 0, backend().cur, m2, h->size, E->rp,
                           h->e_col, (const T*)E->val, h->q, (const T*)rhs->d, (T*)rhs2->d);
        RAMD_HIP(hipGetLastError());
        return RAMD_OK;
    }
    h->down_rhs = nullptr;
    RAMD_TRY(ramd_vec_copy_from_permute(h->rhs_, rhs, h->perm));
    RAMD_TRY(ramd_vec_copy_from_offset(h->x1, h->rhs_, 0, 0, h->size));
    h->down_rhs = rhs;
    if(m2 == 0)
        return RAMD_OK;
    RAMD_TRY(ramd_vec_copy_from_offset(rhs2, h->rhs_, h->size, 0, m2));
    if(h->E->nnz > 0 || h->E->format != RAMD_CSR)
        RAMD_TRY(ramd_mat_apply_add(h->E, h->x1, -1.0, rhs2));
    return RAMD_OK;
}

template <typename T>
int me_up_t(ramd_me_s* h, ramd_vec_t rhs, ramd_vec_t x2, ramd_vec_t x)
{
    const int m2 = h->n - h->size;
    if(h->form == 1)
    {
        const ramd_mat_s* F  = h->F;
        const bool        hf = F && F->nnz > 0;
        hipLaunchKernelGGL((k_me_up<T>), dim3((h->n + kBlock - 1) / kBlock), dim3(kBlock), 0, backend().cur, h->n, h->size,
                           hf ? F->rp : (const int*)nullptr, hf ? F->ci : (const int*)nullptr, hf ? (const T*)F->val : (const T*)nullptr,
                           h->q, (const T*)h->dinv->d, (const T*)rhs->d, m2 > 0 ? (const T*)x2->d : (const T*)nullptr, (T*)x->d);
        RAMD_HIP(hipGetLastError());
        return RAMD_OK;
    }
    if(h->down_rhs != rhs)
        RAMD_FAIL(RAMD_ERR_STATE, "me_up: the stepwise form continues ramd_me_down of the same rhs, and none came before this call");
    h->down_rhs = nullptr; // (x1 is used up)
    if(m2 > 0 && (h->F->nnz > 0 || h->F->format != RAMD_CSR))
        RAMD_TRY(ramd_mat_apply_add(h->F, x2, -1.0, h->x1));
    RAMD_TRY(ramd_vec_pointwise_mult(h->x1, h->dinv));
    RAMD_TRY(ramd_vec_copy_from_offset(h->x_, h->x1, 0, 0, h->size));
    if(m2 > 0)
        RAMD_TRY(ramd_vec_copy_from_offset(h->x_, x2, 0, h->size, m2));
    RAMD_TRY(ramd_vec_copy_from_permute_backward(x, h->x_, h->perm));
    return RAMD_OK;
}

} // namespace

extern "C" {

int ramd_mat_maximal_independent_set(ramd_mat_t m, ramd_vec_t perm, int max_rounds, int* size, int64_t* info)
{
    RAMD_NARROW_ONLY(m);
    if(!m || !perm || !size || max_rounds < 0)
        RAMD_FAIL(RAMD_ERR_ARG, "MaximalIndependentSet: bad arguments");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(perm->dtype != RAMD_I32 || m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "MaximalIndependentSet: a square matrix and an int vector expected");
    return mis_impl(m, perm, max_rounds, size, info);
}

int ramd_mat_compress(ramd_mat_t m, double drop)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null handle");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(m->nnz <= 0) // (host_matrix_csr.cpp:3681)
        return RAMD_OK;
    return compress(m, drop);
}

int ramd_me_build(ramd_mat_t op, double drop_off, int form, int max_rounds, ramd_me_t* out)
{
    RAMD_NARROW_ONLY(op);
    if(!op || !out || form < -1 || form > 1 || max_rounds < 0 || !(drop_off >= 0.0))
        RAMD_FAIL(RAMD_ERR_ARG, "me_build: bad arguments (form is -1 auto, 0 stepwise, 1 fused)");
    if(op->dtype != RAMD_F64 && op->dtype != RAMD_F32)
        RAMD_FAIL(RAMD_ERR_ARG, "me_build: a real operator expected");
    if(op->nrow != op->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "me_build: the operator is not square");
    if(op->nrow <= 0 || (op->format == RAMD_CSR && op->nnz <= 0))
        RAMD_FAIL(RAMD_ERR_ARG, "me_build: the operator is empty");
    ramd_me_s* h = new ramd_me_s;
    h->dtype     = op->dtype;
    h->n         = op->nrow;
    h->form      = form == 1 || (form == -1 && kMeAutoFused) ? 1 : 0;
    ramd_mat_t A = nullptr;
    int        s = ramd_mat_clone(op, &A);
    if(s == RAMD_OK && A->format != RAMD_CSR)
        s = ramd_mat_convert(A, RAMD_CSR);
    if(s == RAMD_OK)
        s = me_build_steps(h, A, drop_off, max_rounds);
    if(A)
        (void)ramd_mat_destroy(A);
    const int m2 = h->n - h->size;
    if(s == RAMD_OK && h->form == 1 && m2 > 0)
    {
        s = dev_alloc(&h->e_col, h->E->nnz);
        if(s == RAMD_OK && h->E->nnz > 0)
        {
            hipLaunchKernelGGL(k_me_map, dim3(ew_grid(h->E->nnz)), dim3(kBlock), 0, backend().cur, h->E->nnz, h->E->ci, h->q, h->e_col);
            if(hipGetLastError() != hipSuccess)
                s = RAMD_ERR_HIP;
        }
    }
    if(s == RAMD_OK && h->form == 0)
    {
        s = me_new_vec(h->dtype, h->n, &h->rhs_);
        if(s == RAMD_OK)
            s = me_new_vec(h->dtype, h->n, &h->x_);
        if(s == RAMD_OK)
            s = me_new_vec(h->dtype, h->size, &h->x1);
    }
    if(s != RAMD_OK)
    {
        h->release();
        delete h;
        return s;
    }
    *out = h;
    return RAMD_OK;
}

int ramd_me_schur(ramd_me_t h, ramd_mat_t* out)
{
    if(!h || !out)
        RAMD_FAIL(RAMD_ERR_ARG, "me_schur: bad arguments");
    if(!h->AA)
        RAMD_FAIL(RAMD_ERR_STATE, "me_schur: the Schur complement was handed out already");
    *out  = h->AA;
    h->AA = nullptr;
    return RAMD_OK;
}

int ramd_me_convert(ramd_me_t h, int format)
{
    if(!h)
        RAMD_FAIL(RAMD_ERR_ARG, "me_convert: null plan");
    if(h->form == 1)
        RAMD_FAIL(RAMD_ERR_STATE, "me_convert: the fused form reads E and F in CSR (build the stepwise form, form = 0)");
    ramd_mat_t ms[] = {h->E, h->F};
    for(ramd_mat_t m : ms)
    {
        if(!m || m->format == format || m->nnz <= 0)
            continue;
        if(m->format != RAMD_CSR && format != RAMD_CSR)
            RAMD_TRY(ramd_mat_convert(m, RAMD_CSR));
        const int s = ramd_mat_convert(m, format);
        if(s != RAMD_OK && s != RAMD_ERR_REFUSED) // (a refused ELL conversion leaves the matrix in CSR, as ConvertTo does)
            return s;
    }
    return RAMD_OK;
}

int ramd_me_down(ramd_me_t h, ramd_vec_t rhs, ramd_vec_t rhs2)
{
    if(!h || !rhs || !rhs2 || rhs == rhs2)
        RAMD_FAIL(RAMD_ERR_ARG, "me_down: bad arguments (rhs and rhs2 must be two vectors)");
    if(rhs->dtype != h->dtype || rhs2->dtype != h->dtype || rhs->n != h->n || rhs2->n != h->n - h->size)
        RAMD_FAIL(RAMD_ERR_ARG, "me_down: vector size / type mismatch");
    return h->dtype == RAMD_F64 ? me_down_t<double>(h, rhs, rhs2) : me_down_t<float>(h, rhs, rhs2);
}

int ramd_me_up(ramd_me_t h, ramd_vec_t rhs, ramd_vec_t x2, ramd_vec_t x)
{
    if(!h || !rhs || !x2 || !x || x == rhs || x == x2)
        RAMD_FAIL(RAMD_ERR_ARG, "me_up: bad arguments (x must not be rhs or x2)");
    if(rhs->dtype != h->dtype || x2->dtype != h->dtype || x->dtype != h->dtype || rhs->n != h->n || x->n != h->n
       || x2->n != h->n - h->size)
        RAMD_FAIL(RAMD_ERR_ARG, "me_up: vector size / type mismatch");
    return h->dtype == RAMD_F64 ? me_up_t<double>(h, rhs, x2, x) : me_up_t<float>(h, rhs, x2, x);
}

int ramd_me_info(ramd_me_t h, int64_t* out8)
{
    if(!h || !out8)
        RAMD_FAIL(RAMD_ERR_ARG, "me_info: bad arguments");
    out8[0] = h->form;
    out8[1] = h->n;
    out8[2] = h->size;
    out8[3] = h->mis_path;
    out8[4] = h->mis_rounds;
    out8[5] = h->mis_sym;
    out8[6] = (h->E ? h->E->nnz : 0) + (h->F ? h->F->nnz : 0);
    out8[7] = h->aa_nnz;
    return RAMD_OK;
}

int ramd_me_destroy(ramd_me_t h)
{
    if(h)
    {
        h->release();
        delete h;
    }
    return RAMD_OK;
}

} // extern "C"
