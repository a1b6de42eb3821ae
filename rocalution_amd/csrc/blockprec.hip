// blockprec.hip -- the BlockPreconditioner on gfx950: the diagonal blocks, the strictly lower block part and the vector work of
// the block forward substitution around the caller's block solvers.
//
// Reference: src/solvers/preconditioners/preconditioner_blockprecond.cpp (Build :188-296, Solve :298-391).
//
// With nb blocks of sizes_b rows, off_b = sum_{k < b} sizes_k and P the operator (permuted as LocalMatrix::Permute does where a
// permutation is set), one apply is
//     rhs' = rhs laid out as CopyFromPermute does, rhs'[perm[i]] = rhs[i]           (no permutation: rhs' = rhs)
//     b = 0 .. nb - 1:   r_b = rhs'[off_b ...) ; r_b += (-1) P_bj z_j for j = 0 .. b - 1 (ApplyAdd) ; z_b = D_b^-1 r_b
//     x[i] = z[perm[i]], z the pieces behind one another (CopyFromPermuteBackward)  (no permutation: x = z)
// SetDiagonalSolver() (diag_only) leaves the ApplyAdd calls out.  ApplyAdd adds term by term INTO the row's element,
// r = r + ((-1) a) z in storage order (host_matrix_csr.cpp:759-767, MODE 1 of spmv.hip), so over the blocks j ascending a row
// of r_b is ONE chain over its entries with a column in front of off_b, block by block.  Two forms:
//   stepwise (form 0)  the blocks P_bj, j < b, ExtractSubMatrix results as the reference keeps them; step b is a slice copy and
//                      b ApplyAdd calls, the join nb slice copies (and the two permutation kernels on a full-length vector)
//   fused    (form 1)  ONE matrix L of n rows: row off_b + l holds the entries of that row of P whose column lies in a block
//                      j < b, global columns, grouped by block ascending and in storage order within a block -- the chain
//                      above as it stands.  Step b is one launch over the rows of block b: it gathers the row's element of rhs
//                      through the inverse permutation, walks the row (the wave-private walk of wave_rows.hpp where the block
//                      row has 16+ entries a row, as k_csr_wr is chosen; lane = row straight from memory below that) and writes
//                      r_b once.  The pieces z_j are nb separate vectors: their pointers and the offsets travel as a kernel
//                      argument (up to kBpMaxPieces; beyond that the plan takes form 0) and are looked up from LDS.  The join
//                      is one launch that writes every element of x once.
// Both forms give the same bits.  form -1: see ramd_bp_build.  The upper blocks are never stored.
#include "csr_filter.hpp"
#include "device_utils.hpp"
#include "matrix_impl.hpp"
#include "wave_rows.hpp"

#include <climits>
#include <string>
#include <vector>

struct ramd_bp_s
{
    int                                  dtype = RAMD_F64;
    int                                  n = 0, nb = 0, form = 0, diag_only = 0;
    int64_t                              l_nnz = 0;
    std::vector<int>                     sizes, off; // off: [nb + 1]
    std::vector<char>                    long_rows; // fused: block row b walks its rows from wave-private LDS images
    int*                                 d_off  = nullptr; // [nb + 1] on the device (the assembly of L)
    int*                                 d_pinv = nullptr; // [n] inverse permutation: rhs'[k] = rhs[pinv[k]]
    ramd_vec_t                           perm   = nullptr; // the plan's own copy of the permutation
    ramd_vec_t                           work   = nullptr; // stepwise with a permutation: the reference's x_
    ramd_mat_t                           L      = nullptr;
    std::vector<ramd_mat_t>              locals; // what ramd_bp_local has not handed out yet
    std::vector<std::vector<ramd_mat_t>> lower; // stepwise: lower[b][j], j < b
    void                                 release()
    {
        ramd::dev_free(&d_off);
        ramd::dev_free(&d_pinv);
        if(perm)
            (void)ramd_vec_destroy(perm);
        if(work)
            (void)ramd_vec_destroy(work);
        if(L)
            (void)ramd_mat_destroy(L);
        perm = work = nullptr;
        L           = nullptr;
        for(ramd_mat_t m : locals)
            if(m)
                (void)ramd_mat_destroy(m);
        locals.clear();
        for(auto& row : lower)
            for(ramd_mat_t m : row)
                if(m)
                    (void)ramd_mat_destroy(m);
        lower.clear();
    }
};

namespace ramd
{

constexpr int kBpMaxPieces = 64; // piece pointers (512 bytes) and offsets (260 bytes) that travel as a kernel argument
constexpr int kBpCap       = 1024; // entries of a wave's LDS image per pass (k_csr_wr's with stored columns: three workgroups per CU)
constexpr int kBpGW        = 14; // gathers in flight per row (k_csr_wr's measured choice)
constexpr int kBpLongRow   = 16; // entries a row from which a block row takes the wave-private walk (as k_csr_wr is chosen)

struct BpTable
{
    int off[kBpMaxPieces + 1];
};
template <typename T>
struct BpPieces
{
    const T* p[kBpMaxPieces];
};

// block of index k over the offsets off[0 .. nb] in memory: the b with off[b] <= k < off[b + 1]
__device__ __forceinline__ int bp_block_of(const int* __restrict__ off, int nb, int k)
{
    int lo = 0, hi = nb;
    while(hi - lo > 1)
    {
        const int mid = (lo + hi) >> 1;
        if(off[mid] <= k)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// the tables of a launch in LDS: soff[j] = off_j for the `cnt` blocks in use, INT_MAX behind them; sp[j] their pieces.  `top`
// is the largest power of two <= cnt - 1 (0 for one block): bp_find then visits soff[j + s] with j + s <= 2 top - 1 < cnt
template <typename T>
__device__ __forceinline__ void bp_stage_tables(const BpTable& tb, const BpPieces<T>& pc, int cnt, int* soff, const T** sp)
{
    if(threadIdx.x < kBpMaxPieces)
    {
        const int t = threadIdx.x;
        soff[t]     = t < cnt ? tb.off[t] : INT_MAX;
        sp[t]       = pc.p[t < cnt ? t : 0];
    }
    __syncthreads();
}
__device__ __forceinline__ int bp_find(const int* soff, int top, int k)
{
    int j = 0;
    for(int s = top; s > 0; s >>= 1)
        j += soff[j + s] <= k ? s : 0;
    return j;
}

// step b, block rows of 16+ entries a row: a wave stages the entries of ITS 64 rows of L and walks them lane = row
// (wave_rows.hpp).  rows [row_lo, row_hi) = [off_b, off_b + sizes_b); pinv == nullptr: no permutation
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bp_step_wave(int row_lo, int row_hi, int b, int top, BpTable tb, const int* __restrict__ rp,
                                                         const int* __restrict__ ci, const T* __restrict__ val,
                                                         const T* __restrict__ rhs, const int* __restrict__ pinv, BpPieces<T> pc,
                                                         T* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char bp_lds[];
    __shared__ int      soff[kBpMaxPieces];
    __shared__ const T* sp[kBpMaxPieces];
    T*   sval_all = reinterpret_cast<T*>(bp_lds); // [4][kBpCap]
    int* scol_all = reinterpret_cast<int*>(bp_lds + sizeof(T) * 4 * kBpCap); // [4][kBpCap]
    bp_stage_tables<T>(tb, pc, b, soff, sp);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = row_lo + blockIdx.x * kBlock + 64 * wave;
    if(row0 >= row_hi) // (wave-uniform; no workgroup barrier behind this point)
        return;
    const int  row   = row0 + lane;
    const bool live  = row < row_hi;
    const int  start = rp[row0];
    const int  end   = rp[min(row0 + 64, row_hi)];
    int        rs = end, re = end;
    T          sum = (T)0;
    if(live)
    {
        rs  = rp[row];
        re  = rp[row + 1];
        sum = rhs[pinv ? pinv[row] : row];
    }
    // the wave's base (wave_rows.hpp): rows and passes are offsets from it
    const int  a0  = start & ~3;
    const T*   vw  = val + a0;
    const int* cw  = ci + a0;
    const int  lrs = rs - a0, lre = re - a0, lend = end - a0;
    T*         sv  = sval_all + wave * kBpCap;
    int*       sc  = scol_all + wave * kBpCap;
    for(int cb = 0; cb < lend; cb += kBpCap)
    {
        wave_stage_pass<T, kBpCap, true>(cw, vw, cb, lend, lane, sc, sv);
        const int lo = max(lrs, cb), hi = min(lre, cb + kBpCap);
        sum = wave_walk_pass<T, kBpGW>(
            sv, lo - cb, hi - lo, sum, [&](int idx, int k, bool& ok) { return sc[idx]; },
            [&](int col) {
                const int j = bp_find(soff, top, col);
                return sp[j][col - soff[j]];
            },
            [&](T s, T a, T z) { return s + (T)(-1) * a * z; }); // (ApplyAdd with the scalar -1, term by term)
    }
    if(live)
        nt_store(sum, out + (row - row_lo));
}

// step b, short rows (and diag_only, rp == nullptr: the slice of rhs' alone): lane = row straight from memory
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bp_step_lane(int row_lo, int row_hi, int b, int top, BpTable tb, const int* __restrict__ rp,
                                                         const int* __restrict__ ci, const T* __restrict__ val,
                                                         const T* __restrict__ rhs, const int* __restrict__ pinv, BpPieces<T> pc,
                                                         T* __restrict__ out)
{
    __shared__ int      soff[kBpMaxPieces];
    __shared__ const T* sp[kBpMaxPieces];
    bp_stage_tables<T>(tb, pc, b, soff, sp);
    const int row = row_lo + blockIdx.x * kBlock + threadIdx.x;
    if(row >= row_hi)
        return;
    T sum = rhs[pinv ? pinv[row] : row];
    if(rp)
    {
        const int e = rp[row + 1];
        for(int k = rp[row]; k < e; ++k)
        {
            const int col = ci[k];
            const int j   = bp_find(soff, top, col);
            sum           = sum + (T)(-1) * val[k] * sp[j][col - soff[j]];
        }
    }
    out[row - row_lo] = sum;
}

// join: x[i] = z[perm[i]] (no permutation: z[i]), z the nb pieces behind one another; every element of x written once
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bp_join(int n, int nb, int top, BpTable tb, const int* __restrict__ perm, BpPieces<T> pc,
                                                    T* __restrict__ x)
{
    __shared__ int      soff[kBpMaxPieces];
    __shared__ const T* sp[kBpMaxPieces];
    bp_stage_tables<T>(tb, pc, nb, soff, sp);
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
    {
        const int k = perm ? perm[i] : (int)i;
        const int j = bp_find(soff, top, k);
        x[i]        = sp[j][k - soff[j]];
    }
}

// the inverse permutation and the check that perm is one: pinv preset to -1; bad[0] = 1 where an index is out of range,
// and (second kernel) where an element of pinv was never written, i.e. another one was written twice
__global__ __launch_bounds__(kBlock) void k_bp_pinv(int n, const int* __restrict__ perm, int* __restrict__ pinv, int* __restrict__ bad)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
    {
        const int p = perm[i];
        if(p < 0 || p >= n)
            bad[0] = 1;
        else
            pinv[p] = (int)i;
    }
}
__global__ __launch_bounds__(kBlock) void k_bp_pinv_check(int n, const int* __restrict__ pinv, int* __restrict__ bad)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
        if(pinv[i] < 0)
            bad[0] = 1;
}

// L: row r of block b keeps the entries with a column in front of off_b (the rule that csr_filter.hpp counts with); they are
// written block by block ascending, in storage order within a block (a pass over the row per block that occurs in it), which
// is not the shared fill; the operator's rows need not be sorted
struct BpLowerRule
{
    static constexpr bool kRowsOnce = true;
    const int*            off;
    int                   nb;
    struct Row
    {
        int src, lim;
    };
    __device__ Row row(int64_t r) const { return Row{(int)r, off[bp_block_of(off, nb, (int)r)]}; }
    template <typename T>
    __device__ bool keep(const Row& r, int col, T) const { return col < r.lim; }
};
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bp_lower_fill(int n, int nb, const int* __restrict__ off, const int* __restrict__ rp,
                                                          const int* __restrict__ ci, const T* __restrict__ val,
                                                          const int* __restrict__ orp, int* __restrict__ oci, T* __restrict__ oval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gsz)
    {
        const int lim = off[bp_block_of(off, nb, (int)r)];
        const int rb = rp[r], re = rp[r + 1];
        int       q    = orp[r];
        int       done = 0; // columns in front of `done` are written
        while(done < lim)
        {
            int first = INT_MAX; // the smallest column not written yet
            for(int j = rb; j < re; ++j)
            {
                const int c = ci[j];
                if(c >= done && c < lim && c < first)
                    first = c;
            }
            if(first == INT_MAX)
                break;
            const int jb = bp_block_of(off, nb, first);
            const int lo = off[jb], hi = off[jb + 1];
            for(int j = rb; j < re; ++j)
            {
                const int c = ci[j];
                if(c >= lo && c < hi)
                {
                    oci[q]  = c;
                    oval[q] = val[j];
                    ++q;
                }
            }
            done = hi;
        }
    }
}

namespace
{

int bp_top(int cnt) // largest power of two <= cnt - 1, 0 for cnt <= 1
{
    int t = 0;
    for(int s = 1; s <= cnt - 1; s <<= 1)
        t = s;
    return t;
}

int bp_check_vec(const ramd_bp_s* h, ramd_vec_t v, int64_t n, const char* what)
{
    if(!v || v->dtype != h->dtype || v->n != n)
        RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": vector size / type mismatch");
    return RAMD_OK;
}
int bp_check_pieces(const ramd_bp_s* h, const ramd_vec_t* p, int cnt, ramd_vec_t a, ramd_vec_t b, const char* what)
{
    if(cnt > 0 && !p)
        RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": one piece vector per earlier block expected");
    for(int i = 0; i < cnt; ++i)
    {
        RAMD_TRY(bp_check_vec(h, p[i], h->sizes[(size_t)i], what));
        if(p[i] == a || p[i] == b)
            RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": a piece must not be the vector read or written beside it");
    }
    return RAMD_OK;
}

// perm -> the plan's copy and its inverse; RAMD_ERR_ARG where it is no permutation of 0 .. n - 1
int bp_take_perm(ramd_bp_s* h, ramd_vec_t perm)
{
    Backend& b = backend();
    RAMD_TRY(ramd_vec_create(RAMD_I32, &h->perm));
    RAMD_TRY(ramd_vec_copy_from(h->perm, perm));
    RAMD_TRY(dev_alloc(&h->d_pinv, h->n));
    int* bad = nullptr;
    RAMD_TRY(dev_alloc(&bad, 1));
    int  flag = 0;
    bool ok   = hipMemsetAsync(h->d_pinv, 0xFF, sizeof(int) * (size_t)h->n, b.cur) == hipSuccess
              && hipMemsetAsync(bad, 0, sizeof(int), b.cur) == hipSuccess;
    if(ok)
    {
        hipLaunchKernelGGL(k_bp_pinv, dim3(ew_grid(h->n)), dim3(kBlock), 0, b.cur, h->n, (const int*)h->perm->d, h->d_pinv, bad);
        hipLaunchKernelGGL(k_bp_pinv_check, dim3(ew_grid(h->n)), dim3(kBlock), 0, b.cur, h->n, (const int*)h->d_pinv, bad);
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&flag, bad, sizeof(int), hipMemcpyDeviceToHost, b.cur) == hipSuccess
             && hipStreamSynchronize(b.cur) == hipSuccess;
    }
    dev_free(&bad);
    if(!ok)
        RAMD_FAIL(RAMD_ERR_HIP, "BlockPreconditioner: inverting the permutation failed");
    if(flag)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: the permutation vector is not a permutation of 0 .. n - 1");
    return RAMD_OK;
}

// the offsets of L (csr_filter.hpp) and its entries, queued on the current stream; *scratch: the caller's to free behind its wait
template <typename T>
int bp_lower_t(ramd_bp_s* h, const ramd_mat_s* P, int** scratch)
{
    const int* off = h->d_off;
    int64_t    nnz = 0;
    RAMD_TRY(csr_filter_offsets("BlockPreconditioner", "the strictly lower block part", BpLowerRule{off, h->nb}, (const int*)P->rp,
                                (const int*)P->ci, (const T*)P->val, h->n, h->n, h->L, &nnz, scratch));
    if(nnz > 0)
        hipLaunchKernelGGL((k_bp_lower_fill<T>), dim3(ew_grid(h->n)), dim3(kBlock), 0, backend().cur, h->n, h->nb, off, (const int*)P->rp,
                           (const int*)P->ci, (const T*)P->val, (const int*)h->L->rp, h->L->ci, (T*)h->L->val);
    return hipGetLastError() == hipSuccess ? RAMD_OK : RAMD_ERR_HIP;
}

// L of the narrow CSR matrix P, and which block rows take the wave-private walk
int bp_assemble_lower(ramd_bp_s* h, const ramd_mat_s* P)
{
    Backend& b = backend();
    RAMD_TRY(ramd_mat_create(h->dtype, &h->L));
    int* scratch = nullptr;
    int  s       = h->dtype == RAMD_F64 ? bp_lower_t<double>(h, P, &scratch) : bp_lower_t<float>(h, P, &scratch);
    // entries of every block row: the row offsets at the block offsets
    std::vector<int> at((size_t)h->nb + 1, 0);
    for(int i = 0; i <= h->nb && s == RAMD_OK; ++i)
        if(hipMemcpyAsync(&at[(size_t)i], h->L->rp + h->off[(size_t)i], sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    if(hipStreamSynchronize(b.cur) != hipSuccess && s == RAMD_OK)
        s = RAMD_ERR_HIP;
    dev_free(&scratch);
    if(s == RAMD_ERR_HIP)
        RAMD_FAIL(s, "BlockPreconditioner: assembling the strictly lower block part failed");
    RAMD_TRY(s);
    h->l_nnz = h->L->nnz;
    h->long_rows.assign((size_t)h->nb, 0);
    for(int i = 0; i < h->nb; ++i)
        h->long_rows[(size_t)i] = at[(size_t)i + 1] - at[(size_t)i] >= (int64_t)kBpLongRow * h->sizes[(size_t)i] ? 1 : 0;
    return RAMD_OK;
}

template <typename T>
int bp_step_t(const ramd_bp_s* h, int b, ramd_vec_t rhs, const ramd_vec_t* z, ramd_vec_t r)
{
    BpTable     tb;
    BpPieces<T> pc;
    for(int i = 0; i <= kBpMaxPieces; ++i)
        tb.off[i] = i <= h->nb ? h->off[(size_t)i] : INT_MAX;
    for(int i = 0; i < kBpMaxPieces; ++i)
        pc.p[i] = i < b ? (const T*)z[i]->d : nullptr;
    const int   lo = h->off[(size_t)b], hi = h->off[(size_t)b + 1];
    const int   cnt  = h->diag_only ? 0 : b;
    const dim3  grid((unsigned)((hi - lo + kBlock - 1) / kBlock)), block(kBlock);
    hipStream_t st = backend().cur;
    const ramd_mat_s* L = h->diag_only ? nullptr : h->L;
    if(L && L->nnz > 0 && h->long_rows[(size_t)b])
        hipLaunchKernelGGL((k_bp_step_wave<T>), grid, block, (sizeof(T) + sizeof(int)) * 4 * (size_t)kBpCap, st, lo, hi, cnt, bp_top(cnt), tb,
                           (const int*)L->rp, (const int*)L->ci, (const T*)L->val, (const T*)rhs->d, (const int*)h->d_pinv, pc, (T*)r->d);
    else
        hipLaunchKernelGGL((k_bp_step_lane<T>), grid, block, 0, st, lo, hi, cnt, bp_top(cnt), tb, L && L->nnz > 0 ? (const int*)L->rp : nullptr,
                           L ? (const int*)L->ci : nullptr, L ? (const T*)L->val : nullptr, (const T*)rhs->d, (const int*)h->d_pinv, pc,
                           (T*)r->d);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

template <typename T>
int bp_join_t(const ramd_bp_s* h, const ramd_vec_t* z, ramd_vec_t x)
{
    BpTable     tb;
    BpPieces<T> pc;
    for(int i = 0; i <= kBpMaxPieces; ++i)
        tb.off[i] = i <= h->nb ? h->off[(size_t)i] : INT_MAX;
    for(int i = 0; i < kBpMaxPieces; ++i)
        pc.p[i] = i < h->nb ? (const T*)z[i]->d : nullptr;
    hipLaunchKernelGGL((k_bp_join<T>), dim3(ew_grid(h->n)), dim3(kBlock), 0, backend().cur, h->n, h->nb, bp_top(h->nb), tb,
                       h->perm ? (const int*)h->perm->d : nullptr, pc, (T*)x->d);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

int bp_build(ramd_bp_s* h, ramd_mat_t op, ramd_vec_t perm)
{
    ramd_mat_t P = op, copy = nullptr;
    int        s = RAMD_OK;
    if(perm)
        s = bp_take_perm(h, perm);
    if(s == RAMD_OK && (perm || op->format != RAMD_CSR))
    {
        s = ramd_mat_clone(op, &copy);
        if(s == RAMD_OK && op->format != RAMD_CSR)
            s = ramd_mat_convert(copy, RAMD_CSR);
        if(s == RAMD_OK && perm)
            s = ramd_mat_permute(copy, h->perm);
        P = copy;
    }
    for(int i = 0; i < h->nb && s == RAMD_OK; ++i)
    {
        ramd_mat_t m = nullptr;
        s            = ramd_mat_create(h->dtype, &m);
        if(s == RAMD_OK)
        {
            h->locals.push_back(m);
            s = ramd_mat_extract_submatrix(P, h->off[(size_t)i], h->off[(size_t)i], h->sizes[(size_t)i], h->sizes[(size_t)i], m);
        }
    }
    if(s == RAMD_OK && !h->diag_only && h->form == 1)
    {
        s = dev_alloc(&h->d_off, (int64_t)h->nb + 1);
        if(s == RAMD_OK
           && hipMemcpy(h->d_off, h->off.data(), sizeof(int) * ((size_t)h->nb + 1), hipMemcpyHostToDevice) != hipSuccess)
            s = RAMD_ERR_HIP;
        if(s == RAMD_OK)
            s = bp_assemble_lower(h, P);
    }
    if(s == RAMD_OK && !h->diag_only && h->form == 0)
    {
        h->lower.resize((size_t)h->nb);
        for(int i = 0; i < h->nb && s == RAMD_OK; ++i)
            for(int j = 0; j < i && s == RAMD_OK; ++j)
            {
                ramd_mat_t m = nullptr;
                s            = ramd_mat_create(h->dtype, &m);
                if(s == RAMD_OK)
                {
                    h->lower[(size_t)i].push_back(m);
                    s = ramd_mat_extract_submatrix(P, h->off[(size_t)i], h->off[(size_t)j], h->sizes[(size_t)i], h->sizes[(size_t)j], m);
                }
            }
    }
    if(s == RAMD_OK && h->form == 0 && h->perm)
    {
        s = ramd_vec_create(h->dtype, &h->work);
        if(s == RAMD_OK)
            s = ramd_vec_allocate(h->work, h->n);
    }
    if(copy)
        (void)ramd_mat_destroy(copy);
    return s;
}

} // namespace
} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_bp_build(ramd_mat_t op, int nb, const int* sizes, ramd_vec_t perm, int diag_only, int form, ramd_bp_t* out)
{
    RAMD_NARROW_ONLY(op);
    if(!op || !out || form < -1 || form > 1)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: bad arguments (form is -1 auto, 0 stepwise, 1 fused)");
    if(op->dtype != RAMD_F64 && op->dtype != RAMD_F32)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: a real operator expected");
    if(op->nrow != op->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: the operator is not square");
    if(nb < 1 || !sizes)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: the number of blocks must be at least 1 (got " + std::to_string(nb) + ")");
    int64_t sum = 0;
    for(int i = 0; i < nb; ++i)
    {
        if(sizes[i] < 1)
            RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: block " + std::to_string(i) + " has size " + std::to_string(sizes[i])
                                        + " (every block needs at least one row)");
        sum += sizes[i];
    }
    if(sum != op->nrow)
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: the block sizes sum to " + std::to_string(sum) + ", the operator has "
                                    + std::to_string(op->nrow) + " rows");
    if(perm && (perm->dtype != RAMD_I32 || perm->n != op->nrow))
        RAMD_FAIL(RAMD_ERR_ARG, "BlockPreconditioner: the permutation must be an int32 vector of length " + std::to_string(op->nrow)
                                    + " (got length " + std::to_string(perm->n) + ")");
    ramd_bp_s* h = new ramd_bp_s;
    h->dtype     = op->dtype;
    h->n         = op->nrow;
    h->nb        = nb;
    h->diag_only = diag_only ? 1 : 0;
    // form -1: the fused form (tools/blockprec_measure.py, profiles/blockprec.md); more blocks than piece pointers travel as a
    // kernel argument: the stepwise calls, whatever was asked for
    h->form = form == -1 ? 1 : form;
    if(nb > kBpMaxPieces)
        h->form = 0;
    h->sizes.assign(sizes, sizes + nb);
    h->off.assign((size_t)nb + 1, 0);
    for(int i = 0; i < nb; ++i)
        h->off[(size_t)i + 1] = h->off[(size_t)i] + sizes[i];
    const int s = bp_build(h, op, perm);
    if(s != RAMD_OK)
    {
        h->release();
        delete h;
        return s;
    }
    *out = h;
    return RAMD_OK;
}

int ramd_bp_local(ramd_bp_t h, int block, ramd_mat_t* out)
{
    if(!h || !out || block < 0 || block >= (int)h->locals.size())
        RAMD_FAIL(RAMD_ERR_ARG, "bp_local: bad arguments");
    if(!h->locals[(size_t)block])
        RAMD_FAIL(RAMD_ERR_STATE, "bp_local: this diagonal block was handed out already");
    *out                     = h->locals[(size_t)block];
    h->locals[(size_t)block] = nullptr;
    return RAMD_OK;
}

int ramd_bp_step(ramd_bp_t h, int b, ramd_vec_t rhs, const ramd_vec_t* z, ramd_vec_t r)
{
    if(!h || b < 0 || b >= h->nb || rhs == r)
        RAMD_FAIL(RAMD_ERR_ARG, "bp_step: bad arguments (block 0 .. nb - 1; rhs and r must be two vectors)");
    RAMD_TRY(bp_check_vec(h, rhs, h->n, "bp_step"));
    RAMD_TRY(bp_check_vec(h, r, h->sizes[(size_t)b], "bp_step"));
    const int cnt = h->diag_only ? 0 : b;
    RAMD_TRY(bp_check_pieces(h, z, cnt, rhs, r, "bp_step"));
    if(h->form == 1)
        return h->dtype == RAMD_F64 ? bp_step_t<double>(h, b, rhs, z, r) : bp_step_t<float>(h, b, rhs, z, r);
    // (preconditioner_blockprecond.cpp:312-326, :344-353) the permuted copy of rhs is made at block 0 and serves the blocks
    // behind it: the steps of one apply run b = 0 .. nb - 1 on one rhs
    if(h->perm && b == 0)
        RAMD_TRY(ramd_vec_copy_from_permute(h->work, rhs, h->perm));
    RAMD_TRY(ramd_vec_copy_from_offset(r, h->perm ? h->work : rhs, h->off[(size_t)b], 0, h->sizes[(size_t)b]));
    for(int j = 0; j < cnt; ++j)
        RAMD_TRY(ramd_mat_apply_add(h->lower[(size_t)b][(size_t)j], z[j], -1.0, r));
    return RAMD_OK;
}

int ramd_bp_join(ramd_bp_t h, const ramd_vec_t* z, int nb, ramd_vec_t x)
{
    if(!h || nb != h->nb)
        RAMD_FAIL(RAMD_ERR_ARG, "bp_join: one piece vector per block expected");
    RAMD_TRY(bp_check_vec(h, x, h->n, "bp_join"));
    RAMD_TRY(bp_check_pieces(h, z, nb, x, x, "bp_join"));
    if(h->form == 1)
        return h->dtype == RAMD_F64 ? bp_join_t<double>(h, z, x) : bp_join_t<float>(h, z, x);
    ramd_vec_t to = h->perm ? h->work : x; // (:373-389)
    for(int i = 0; i < nb; ++i)
        RAMD_TRY(ramd_vec_copy_from_offset(to, z[i], 0, h->off[(size_t)i], h->sizes[(size_t)i]));
    if(h->perm)
        RAMD_TRY(ramd_vec_copy_from_permute_backward(x, h->work, h->perm));
    return RAMD_OK;
}

int ramd_bp_info(ramd_bp_t h, int64_t* out8)
{
    if(!h || !out8)
        RAMD_FAIL(RAMD_ERR_ARG, "bp_info: bad arguments");
    int big = 0, small = INT_MAX;
    for(int s : h->sizes)
    {
        big   = s > big ? s : big;
        small = s < small ? s : small;
    }
    out8[0] = h->form;
    out8[1] = h->nb;
    out8[2] = h->n;
    out8[3] = h->l_nnz;
    out8[4] = h->diag_only;
    out8[5] = h->perm ? 1 : 0;
    out8[6] = big;
    out8[7] = small;
    return RAMD_OK;
}

int ramd_bp_piece_cap(void)
{
    return kBpMaxPieces;
}

int ramd_bp_destroy(ramd_bp_t h)
{
    if(h)
    {
        h->release();
        delete h;
    }
    return RAMD_OK;
}

} // extern "C"
