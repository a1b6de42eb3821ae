// spmv_wide.hip -- the products of a CSR matrix with 64-bit row offsets (more than INT32_MAX entries) on gfx950.
//
// The counterpart of the reference built with BUILD_PTRTYPE_64 (CMakeLists.txt:77, src/utils/types.hpp.in:30-32): PtrType is
// int64_t, column indices and row counts stay int.  Arithmetic as in spmv.hip: every row is summed left to right in storage
// order (src/base/host/host_matrix_csr.cpp:702-769), no FMA contraction, so the results equal the narrow kernels' bit for bit.
//
// One kernel, k_csr_wide: the wave-private row walk of k_csr_wr (spmv.hip) restated over a 64-bit block base.  val / ci of
// such a matrix are larger than 4 GiB, so nothing here addresses them by a 32-bit offset from the array base: a wave forms
// ONE 64-bit base -- blk_rp64[block] + the offset of its first row, rounded down to a 16-byte packet -- and everything inside
// its loops is a 32-bit offset from that (mat_wide_finish refuses a 256-row block of 2^31 entries).  Per row the kernel reads
// 4 bytes of offset (row_off, relative to the block) as the narrow kernels read rp, plus 8 bytes per 256 rows (blk_rp64): the
// byte accounting stays the reference's 4 (n + nnz) + 8 (2 n + nnz) (clients/samples/benchmark.cpp:213-233); with row
// patterns the 4 bytes per entry of ci are replaced by one byte per row as in k_csr_wr<PAT>.
// It handles any row length: a wave stages the entries of its 64 rows in passes of kWideCap and lane = row walks them; an
// empty row has nothing to walk, a row longer than a pass is walked across passes.
#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <algorithm>

namespace ramd
{

template <typename T>
struct WidePk;
template <>
struct WidePk<double>
{
    using type             = v2f64;
    static constexpr int N = 2;
};
template <>
struct WidePk<float>
{
    using type             = v4f32;
    static constexpr int N = 4;
};

struct WideWs // the epilogues: fused <dotv or x, y> (one partial per wave, as the narrow kernels), Jacobi sweep
{
    double*     part1;
    const void* dotv;
    const void* jdinv;
    const void* jrhs;
};

// entries of a wave's LDS image per pass (k_csr_wr's: 8 bytes an entry with row patterns, 12 with the stored columns)
template <bool PAT>
constexpr int kWideCapOf = PAT ? 2048 : 1024;
constexpr int kWideGW    = 14; // x gathers in flight per row (k_csr_wr's measured choice)

// MODE 0: y = A x   1: y += scalar A x   2: damped-Jacobi sweep y = x + scalar dinv (rhs - A x)   DOT: partials of <dotv or x, y>
template <typename T, int MODE, bool DOT, bool PAT>
__global__ __launch_bounds__(kBlock) void k_csr_wide(int nrow, int nblk, int per_xcd, const int64_t* __restrict__ blk_rp64,
                                                     const uint32_t* __restrict__ row_off, const int* __restrict__ ci,
                                                     const T* __restrict__ val, const T* __restrict__ x, T* __restrict__ y, T scalar,
                                                     WideWs ws, CsrPattern pat)
{
    using VP           = typename WidePk<T>::type;
    constexpr int VN   = WidePk<T>::N;
    constexpr int kCap = kWideCapOf<PAT>;
    constexpr int GW   = kWideGW;
    extern __shared__ __attribute__((aligned(16))) char wide_lds[];
    T*   sval_all = reinterpret_cast<T*>(wide_lds); // [4][kCap]
    int* scol     = reinterpret_cast<int*>(wide_lds + sizeof(T) * 4 * kCap); // PAT: the dictionary; else [4][kCap] columns
    const int blk = xcd_block(nblk, per_xcd, BandMap{0, 0, 0});
    double    dacc = 0.0;
    if(blk >= 0)
    {
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int row  = blk * 256 + 64 * wave + lane;
        if(PAT)
        {
            for(int i = threadIdx.x; i < pat.n * pat.w; i += kBlock)
                scol[i] = pat.dict[i];
            __syncthreads();
        }
        // the block's entries: [base, base + bend) of ci / val; bend < 2^31 (mat_wide_finish)
        const int64_t base = blk_rp64[blk];
        const int     bend = (int)(blk_rp64[blk + 1] - base);
        int           rs = bend, re = bend; // (a lane behind the last row: an empty row at the block's end)
        if(row < nrow)
        {
            rs = (int)row_off[row];
            re = (threadIdx.x == kBlock - 1 || row + 1 == nrow) ? bend : (int)row_off[row + 1];
        }
        const int start = __builtin_amdgcn_readfirstlane(rs);
        const int end   = __builtin_amdgcn_readlane(re, 63);
        // the wave's 64-bit base, once: its first entry rounded down to a 16-byte packet of both arrays; rows and passes are
        // 32-bit offsets from it
        const int64_t a0    = (base + start) & ~(int64_t)3;
        const T*      vw    = val + a0;
        const int*    cw    = ci + a0;
        const int     shift = (int)(base - a0);
        const int     lrs = rs + shift, lre = re + shift, lend = end + shift;
        int           dbase = 0;
        if(PAT && row < nrow)
            dbase = (int)pat.id[row] * pat.w - lrs;
        T*   sv   = sval_all + wave * kCap;
        int* sc   = scol + wave * kCap;
        T    sum  = (T)0;
        T    xrow = (T)0;
        if(MODE == 1 && row < nrow)
            sum = y[row];
        if(((DOT && !ws.dotv) || MODE == 2) && row < nrow)
            xrow = x[row];
        for(int cb = 0; cb < lend; cb += kCap)
        {
            v4i32 c[kCap / (4 * 64)];
            VP    a[kCap / (VN * 64)];
#pragma unroll
            for(int k = 0; k < (PAT ? 0 : kCap / (4 * 64)); ++k)
            {
                // (every lane loads: a packet behind the wave's entries re-reads the pass's first one)
                const int j = cb + (k * 64 + lane) * 4;
                c[k]        = nt_load(reinterpret_cast<const v4i32*>(cw + (j < lend ? j : cb)));
            }
#pragma unroll
            for(int k = 0; k < kCap / (VN * 64); ++k)
            {
                const int j = cb + (k * 64 + lane) * VN;
                a[k]        = nt_load(reinterpret_cast<const VP*>(vw + (j < lend ? j : cb)));
            }
#pragma unroll
            for(int k = 0; k < (PAT ? 0 : kCap / (4 * 64)); ++k)
            {
                const int g = (k * 64 + lane) * 4;
                if(cb + g < lend)
                    *reinterpret_cast<v4i32*>(sc + g) = c[k];
            }
#pragma unroll
            for(int k = 0; k < kCap / (VN * 64); ++k)
            {
                const int g = (k * 64 + lane) * VN;
                if(cb + g < lend)
                    *reinterpret_cast<VP*>(sv + g) = a[k];
            }
            __builtin_amdgcn_wave_barrier();
            const int lo = max(lrs, cb), hi = min(lre, cb + kCap);
            const int len = hi - lo;
            // no load under a branch: a lane past its row's end reads entry 0 / x[0] and keeps its sum by a select
            for(int jb = 0; __ballot(jb < len) != 0ull; jb += GW)
            {
                int  cc[GW];
                T    v[GW], xv[GW];
                bool ok[GW];
#pragma unroll
                for(int e = 0; e < GW; ++e)
                {
                    ok[e]         = jb + e < len;
                    const int idx = ok[e] ? lo - cb + jb + e : 0;
                    v[e]          = sv[idx];
                    const int col = PAT ? row + scol[ok[e] ? dbase + lo + jb + e : 0] : sc[idx];
                    cc[e]         = ok[e] ? col : 0;
                }
#pragma unroll
                for(int e = 0; e < GW; ++e)
                    xv[e] = x[cc[e]];
#pragma unroll
                for(int e = 0; e < GW; ++e)
                {
                    const T s2 = MODE != 1 ? sum + v[e] * xv[e] : sum + scalar * v[e] * xv[e];
                    sum        = ok[e] ? s2 : sum;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if(row < nrow)
        {
            if(MODE == 2)
            {
                T t = (T)(-1) * sum + static_cast<const T*>(ws.jrhs)[row];
                t   = static_cast<const T*>(ws.jdinv)[row] * t;
                sum = xrow + scalar * t;
            }
            nt_store(sum, y + row);
            if(DOT)
                dacc = (double)sum * (double)(ws.dotv ? static_cast<const T*>(ws.dotv)[row] : xrow);
        }
    }
    if(DOT)
    {
        // one partial per wave in the narrow kernels' places; reduce_sum_to_slot adds them in their fixed order
        const double wsum = wave_reduce_sum(dacc);
        if((threadIdx.x & 63) == 0 && blk >= 0)
            ws.part1[blk * (kBlock / 64) + (threadIdx.x >> 6)] = wsum;
    }
}

template <typename T>
int launch_csr_wide(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv, const T* jdinv,
                    const T* jrhs)
{
    Backend& b = backend();
    if(!m->rp64 || !m->blk_rp64 || !m->row_off)
        RAMD_FAIL(RAMD_ERR_STATE, "wide CSR product: the compact row offsets are missing");
    // row patterns as for the narrow product: analysed once, on the first product of a matrix with >= 2^20 entries
    // (RAMD_CSR_PAT=1: every matrix, =0: never)
    static const int pat_env = getenv("RAMD_CSR_PAT") ? atoi(getenv("RAMD_CSR_PAT")) : -1;
    if(m->pat_state == 0 && pat_env != 0 && (pat_env > 0 || csr_patv_env() > 0 || m->nnz >= (1 << 20)))
        RAMD_TRY(csr_analyse_pattern(const_cast<ramd_mat_s*>(m)));
    const bool       use_pat = pat_env != 0 && m->pat_state == 1 && !m->pat_off;
    if(use_pat) // values from the dictionary too: the narrow matrices' kernel, which reads no row offsets (spmv.hip, k_csr_patv)
    {
        bool taken = false;
        RAMD_TRY(launch_csr_patv<T>(m, x, y, mode, scalar, dot, slot, dotv, jdinv, jrhs, &taken));
        if(taken)
            return RAMD_OK;
    }
    const CsrPattern pat     = {use_pat ? m->pat_id : nullptr, use_pat ? m->pat_dict : nullptr, m->pat_n, m->pat_w};
    const int        nblk    = (m->nrow + 255) / 256;
    const int        per_xcd = (nblk + 7) / 8;
    const int        grid    = per_xcd * 8;
    const size_t lds_pat = sizeof(T) * 4 * kWideCapOf<true> + sizeof(int) * (size_t)kPatMax * kPatMaxW;
    const size_t lds_col = (sizeof(T) + sizeof(int)) * 4 * kWideCapOf<false>;
    static bool  raised  = false; // (more than 64 KB of LDS per workgroup: opt in once per instantiation)
    if(!raised)
    {
#define WIDE_RAISE(MODE, DOT) \
    RAMD_HIP(hipFuncSetAttribute((const void*)k_csr_wide<T, MODE, DOT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pat))
        WIDE_RAISE(0, false);
        WIDE_RAISE(0, true);
        WIDE_RAISE(1, false);
        WIDE_RAISE(2, false);
#undef WIDE_RAISE
        raised = true;
    }
    WideWs ws = {};
    if(dot)
    {
        ramd_mat_s* mm = const_cast<ramd_mat_s*>(m);
        if(!mm->dot_part1 || mm->dot_nblk != nblk)
        {
            dev_free(&mm->dot_part1);
            RAMD_TRY(dev_alloc(&mm->dot_part1, (int64_t)nblk * (kBlock / 64)));
            mm->dot_nblk = nblk;
        }
        ws.part1 = mm->dot_part1;
        ws.dotv  = dotv;
    }
    ws.jdinv = jdinv;
    ws.jrhs  = jrhs;
    if(dot) // (the plain product and the sweep are bracketed by their callers, as in spmv.hip)
        prof_spmv_begin();
#define WIDE_LAUNCH(MODE, DOT)                                                                                                   \
    do                                                                                                                           \
    {                                                                                                                            \
        if(use_pat)                                                                                                              \
            hipLaunchKernelGGL((k_csr_wide<T, MODE, DOT, true>), dim3(grid), dim3(kBlock), lds_pat, b.cur, m->nrow, nblk, per_xcd, \
                               m->blk_rp64, m->row_off, m->ci, (const T*)m->val, x, y, scalar, ws, pat);                         \
        else                                                                                                                     \
            hipLaunchKernelGGL((k_csr_wide<T, MODE, DOT, false>), dim3(grid), dim3(kBlock), lds_col, b.cur, m->nrow, nblk, per_xcd, \
                               m->blk_rp64, m->row_off, m->ci, (const T*)m->val, x, y, scalar, ws, pat);                         \
    } while(0)
    if(mode == 2)
        WIDE_LAUNCH(2, false);
    else if(mode == 0 && !dot)
        WIDE_LAUNCH(0, false);
    else if(mode == 0 && dot)
        WIDE_LAUNCH(0, true);
    else
        WIDE_LAUNCH(1, false);
#undef WIDE_LAUNCH
    const hipError_t e = hipGetLastError();
    if(dot)
        prof_spmv_end();
    RAMD_HIP(e);
    if(dot)
        return reduce_sum_to_slot(ws.part1, (int64_t)nblk * (kBlock / 64), slot);
    return RAMD_OK;
}
template int launch_csr_wide<double>(const ramd_mat_s*, const double*, double*, int, double, bool, int, const double*, const double*,
                                     const double*);
template int launch_csr_wide<float>(const ramd_mat_s*, const float*, float*, int, float, bool, int, const float*, const float*,
                                    const float*);

} // namespace ramd
