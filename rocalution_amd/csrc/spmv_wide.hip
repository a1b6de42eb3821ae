// spmv_wide.hip -- the products of a CSR matrix with 64-bit row offsets (more than INT32_MAX entries) on gfx950.
//
// The counterpart of the reference built with BUILD_PTRTYPE_64 (CMakeLists.txt:77, src/utils/types.hpp.in:30-32): PtrType is
// int64_t, column indices and row counts stay int.  Arithmetic as in spmv.hip: every row is summed left to right in storage
// order (src/base/host/host_matrix_csr.cpp:702-769), no FMA contraction, so the results equal the narrow kernels' bit for bit.
//
// One kernel, k_csr_wide: the wave-private row walk of wave_rows.hpp, shared with k_csr_wr (spmv.hip).  val / ci of such a
// matrix are larger than 4 GiB, so nothing addresses them by a 32-bit offset from the array base: a wave forms ONE 64-bit
// base -- blk_rp64[block] + the offset of its first row, rounded down to a 16-byte packet -- and everything inside
// its loops is a 32-bit offset from that (mat_wide_finish refuses a 256-row block of 2^31 entries).  Per row the kernel reads
// 4 bytes of offset (row_off, relative to the block) as the narrow kernels read rp, plus 8 bytes per 256 rows (blk_rp64): the
// byte accounting stays the reference's 4 (n + nnz) + 8 (2 n + nnz) (clients/samples/benchmark.cpp:213-233); with row
// patterns the 4 bytes per entry of ci are replaced by one byte per row as in k_csr_wr<PAT>.
// It handles any row length: a wave stages the entries of its 64 rows in passes of kWideCap and lane = row walks them; an
// empty row has nothing to walk, a row longer than a pass is walked across passes.
#include "device_utils.hpp"
#include "matrix_impl.hpp"
#include "wave_rows.hpp"

#include <algorithm>

namespace ramd
{

// entries of a wave's LDS image per pass (k_csr_wr's: 8 bytes an entry with row patterns, 12 with the stored columns)
template <bool PAT>
constexpr int kWideCapOf = PAT ? 2048 : 1024;
constexpr int kWideGW    = 14; // x gathers in flight per row (k_csr_wr's measured choice)

// MODE 0: y = A x   1: y += scalar A x   2: damped-Jacobi sweep y = x + scalar dinv (rhs - A x)   DOT: partials of <dotv or x, y>
template <typename T, int MODE, bool DOT, bool PAT>
__global__ __launch_bounds__(kBlock) void k_csr_wide(int nrow, int nblk, int per_xcd, const int64_t* __restrict__ blk_rp64,
                                                     const uint32_t* __restrict__ row_off, const int* __restrict__ ci,
                                                     const T* __restrict__ val, const T* __restrict__ x, T* __restrict__ y, T scalar,
                                                     CsrDotWs ws, CsrPattern pat)
{
    constexpr int kCap = kWideCapOf<PAT>;
    extern __shared__ __attribute__((aligned(16))) char wide_lds[];
    T*   sval_all = reinterpret_cast<T*>(wide_lds); // [4][kCap]
    int* scol     = reinterpret_cast<int*>(wide_lds + sizeof(T) * 4 * kCap); // PAT: the dictionary; else [4][kCap] columns
    const int blk = xcd_block(nblk, per_xcd, BandMap{0, 0, 0});
    if(blk < 0) // (workgroup-uniform)
        return;
    const int  wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int  row  = blk * 256 + 64 * wave + lane;
    const bool live = row < nrow;
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
    if(live)
    {
        rs = (int)row_off[row];
        re = (threadIdx.x == kBlock - 1 || row + 1 == nrow) ? bend : (int)row_off[row + 1];
    }
    const int start = __builtin_amdgcn_readfirstlane(rs);
    const int end   = __builtin_amdgcn_readlane(re, 63);
    // the wave's 64-bit base, once (wave_rows.hpp): rows and passes are 32-bit offsets from it
    const int64_t a0    = (base + start) & ~(int64_t)3;
    const T*      vw    = val + a0;
    const int*    cw    = ci + a0;
    const int     shift = (int)(base - a0);
    const int     lrs = rs + shift, lre = re + shift, lend = end + shift;
    int           dbase = 0;
    if(PAT && live)
        dbase = (int)pat.id[row] * pat.w - lrs;
    T*   sv   = sval_all + wave * kCap;
    int* sc   = scol + wave * kCap;
    T    sum  = (T)0;
    T    xrow = (T)0;
    if(MODE == 1 && live)
        sum = y[row];
    if(((DOT && !ws.dotv) || MODE == 2) && live)
        xrow = x[row];
    for(int cb = 0; cb < lend; cb += kCap)
    {
        wave_stage_pass<T, kCap, !PAT>(cw, vw, cb, lend, lane, sc, sv);
        sum = csr_walk_pass<T, MODE, PAT, kWideGW>(sv, sc, scol, row, dbase, max(lrs, cb), min(lre, cb + kCap), cb, x, scalar, sum);
    }
    csr_row_epilogue<T, MODE, DOT>(live, blk, row, sum, xrow, y, scalar, ws);
}

// (the plain product and the sweep are bracketed by their callers, the fused dot by launch_csr, which also owns ws: spmv.hip)
template <typename T>
int launch_csr_wide(const ramd_mat_s* m, bool use_pat, const T* x, T* y, int mode, bool dot, T scalar, const CsrDotWs& ws)
{
    Backend&         b       = backend();
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
    with_mode_dot<true>(mode, dot, [&](auto M, auto D) {
        constexpr int  MODE = decltype(M)::value;
        constexpr bool DOT  = decltype(D)::value;
        if(use_pat)
            hipLaunchKernelGGL((k_csr_wide<T, MODE, DOT, true>), dim3(grid), dim3(kBlock), lds_pat, b.cur, m->nrow, nblk, per_xcd,
                               m->blk_rp64, m->row_off, m->ci, (const T*)m->val, x, y, scalar, ws, pat);
        else
            hipLaunchKernelGGL((k_csr_wide<T, MODE, DOT, false>), dim3(grid), dim3(kBlock), lds_col, b.cur, m->nrow, nblk, per_xcd,
                               m->blk_rp64, m->row_off, m->ci, (const T*)m->val, x, y, scalar, ws, pat);
    });
    return RAMD_OK;
}
template int launch_csr_wide<double>(const ramd_mat_s*, bool, const double*, double*, int, bool, double, const CsrDotWs&);
template int launch_csr_wide<float>(const ramd_mat_s*, bool, const float*, float*, int, bool, float, const CsrDotWs&);

} // namespace ramd
