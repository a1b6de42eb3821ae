// mcsr.hip -- the MCSR format (modified CSR): CSR <-> MCSR on the device and the diagonal-first products.
//
// Replaces csr_to_mcsr / mcsr_to_csr (src/base/host/host_conversion.cpp:146-323) and HostMatrixMCSR::Apply / ApplyAdd
// (src/base/host/host_matrix_mcsr.cpp:421-494).  Layout, square matrices only, nnz as in CSR:
//     val[0 .. n)                                    the diagonal
//     row_offset[i] = n + csr_row_offset[i] - i      (row_offset[0] = n, row_offset[n] = nnz)
//     col / val [row_offset[i], row_offset[i + 1])   row i's off-diagonal entries in their CSR storage order
//     col[0 .. n)                                    zero, never read
// include/rocalution_amd.h has the refusals and the one deliberate departure from the reference.
//
// The products.  The host loop starts a row's sum with val[i] * x[i] -- no leading 0 + -- and adds the off-diagonal entries in
// storage order, so the result differs from the CSR product in the last bit and in the sign of a zero: a kernel of its own.
// One row per lane, 64 rows per wave.  The lane's two diagonal operands are val[row] and x[row], two fully coalesced loads
// issued before anything else.  The off-diagonal entries of a wave's 64 rows are one contiguous range
// [row_offset[row0], row_offset[row0 + 64)): they go through the wave-private row walk of wave_rows.hpp (wave_stage_pass /
// csr_walk_pass with the stored columns), which k_csr_wr, k_csr_wide and k_tns_tri share -- no workgroup barrier, no load under
// a branch, the sum left to right in storage order, rows longer than a pass of kMcsrCap entries continued across passes.  The
// walk takes the row's initial sum as an argument, so the diagonal-first start needs nothing new in it.
#include "device_utils.hpp"
#include "matrix_impl.hpp"
#include "wave_rows.hpp"

#include <algorithm>
#include <climits>
#include <vector>

namespace ramd
{

// ---------------------------------------------------------------------------------------------------- CSR -> MCSR
// host_conversion.cpp:165-185 counts the diagonal entries of the whole matrix; here per row, and a row that does not store
// exactly one raises the flag (every writer stores the same word)
__global__ __launch_bounds__(kBlock) void k_mcsr_flag(int n, const int* __restrict__ rp, const int* __restrict__ ci, int* __restrict__ bad)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz)
    {
        int nd = 0;
        for(int j = rp[row]; j < rp[row + 1]; ++j)
            nd += ci[j] == row ? 1 : 0;
        if(nd != 1)
            *bad = 1;
    }
}
// host_conversion.cpp:197-225: the offsets are an affine function of the CSR offsets (no scan); one thread walks a row front
// to back, the diagonal entry to val[row], the others to the row's range in their order
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mcsr_fill(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                                      const T* __restrict__ val, int* __restrict__ ro, int* __restrict__ mci,
                                                      T* __restrict__ mval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row <= n; row += gsz)
    {
        const int lo = rp[row];
        ro[row]      = (int)(n + lo - row);
        if(row == n)
            continue;
        int q = (int)(n + lo - row);
        for(int j = lo; j < rp[row + 1]; ++j)
        {
            const int c = ci[j];
            const T   v = val[j];
            if(c == row)
                mval[row] = v;
            else
            {
                mci[q]  = c;
                mval[q] = v;
                ++q;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- MCSR -> CSR
// host_conversion.cpp:263-320: the off-diagonal entries in their order, the diagonal (row, val[row]) appended last, then the
// row sorted ascending by column, stably (the reference's bubble sort swaps on strict >; an insertion sort that moves on
// strict > gives the same order).  Nothing is dropped.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mcsr2csr(int n, const int* __restrict__ ro, const int* __restrict__ mci,
                                                     const T* __restrict__ mval, int* __restrict__ rp, int* __restrict__ ci,
                                                     T* __restrict__ val)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row <= n; row += gsz)
    {
        const int lo = ro[row];
        const int q0 = (int)(lo - n + row);
        rp[row]      = q0;
        if(row == n)
            continue;
        const int len = ro[row + 1] - lo;
        for(int k = 0; k <= len; ++k)
        {
            const int c = k < len ? mci[lo + k] : (int)row;
            const T   v = k < len ? mval[lo + k] : mval[row];
            int       p = q0 + k;
            while(p > q0 && ci[p - 1] > c)
            {
                ci[p]  = ci[p - 1];
                val[p] = val[p - 1];
                --p;
            }
            ci[p]  = c;
            val[p] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- diagonal
// ExtractDiagonal / ExtractInverseDiagonal of an MCSR operator: val[0 .. n), with k_csr_diag's reciprocal rule (a zero gives 1)
template <typename T, bool INV>
__global__ __launch_bounds__(kBlock) void k_mcsr_diag(int n, const T* __restrict__ mval, T* __restrict__ d)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz)
    {
        const T a = mval[row];
        d[row]    = !INV ? a : (a != (T)0 ? (T)1 / a : (T)1);
    }
}

// ---------------------------------------------------------------------------------------------------- products
// entries of a wave's LDS image per pass: k_csr_wr's with the stored columns (12 bytes an entry in fp64, 48 KB a workgroup)
constexpr int kMcsrCap = 1024;

// MODE 0: y = A x (DOT: and one partial of <dotv or x, y> per wave); MODE 1: y += (scalar * a) * x, the diagonal first
template <typename T, int MODE, bool DOT, int GW>
__global__ __launch_bounds__(kBlock) void k_mcsr(int n, const int* __restrict__ ro, const int* __restrict__ ci,
                                                 const T* __restrict__ val, const T* __restrict__ x, T* __restrict__ y, T scalar,
                                                 CsrDotWs ws)
{
    __shared__ __attribute__((aligned(16))) T   sval_all[4 * kMcsrCap];
    __shared__ __attribute__((aligned(16))) int scol_all[4 * kMcsrCap];
    const int  blk  = blockIdx.x;
    const int  wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int  w0   = blk * kBlock + 64 * wave;
    const int  row  = w0 + lane;
    const bool live = row < n;
    // the diagonal term's operands: lane = row, contiguous (a lane behind the last row reads row 0's and keeps nothing)
    const T dv   = val[live ? row : 0];
    const T xrow = x[live ? row : 0];
    int     rs = 0, re = 0;
    if(live)
    {
        rs = ro[row];
        re = ro[row + 1];
    }
    const int start = __builtin_amdgcn_readfirstlane(ro[min(w0, n)]);
    const int end   = __builtin_amdgcn_readfirstlane(ro[min(w0 + 64, n)]);
    // the wave's base (wave_rows.hpp): rows and passes are offsets from it.  A wave without off-diagonal entries stages nothing
    const int  a0   = start & ~3;
    const T*   vw   = val + a0;
    const int* cw   = ci + a0;
    const int  lrs = rs - a0, lre = re - a0, lend = end > start ? end - a0 : 0;
    T*         sv  = sval_all + wave * kMcsrCap;
    int*       sc  = scol_all + wave * kMcsrCap;
    T          sum;
    if(MODE == 1) // host_matrix_mcsr.cpp:485: out[i] += scalar * val[i] * in[i]
    {
        const T y0 = live ? y[row] : (T)0;
        sum        = y0 + scalar * dv * xrow;
    }
    else // :446: sum = val[i] * in[i]
        sum = dv * xrow;
    for(int cb = 0; cb < lend; cb += kMcsrCap)
    {
        wave_stage_pass<T, kMcsrCap, true>(cw, vw, cb, lend, lane, sc, sv);
        sum = csr_walk_pass<T, MODE, false, GW>(sv, sc, sc, row, 0, max(lrs, cb), min(lre, cb + kMcsrCap), cb, x, scalar, sum);
    }
    csr_row_epilogue<T, MODE, DOT>(live, blk, row, sum, xrow, y, scalar, ws);
}

template <typename T>
int launch_mcsr(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv)
{
    Backend& b = backend();
    if(m->format != RAMD_MCSR || m->nrow != m->ncol || m->nrow <= 0 || m->nnz < m->nrow || !m->mcsr_ro || !m->mcsr_ci || !m->mcsr_val)
        RAMD_FAIL(RAMD_ERR_STATE, "MCSR product: the matrix holds no MCSR data (internal)");
    if(dot && mode != 0)
        RAMD_FAIL(RAMD_ERR_ARG, "MCSR product: the fused dot goes with y = A x only (internal)");
    const int grid  = (int)(((int64_t)m->nrow + kBlock - 1) / kBlock);
    const int npart = grid * (kBlock / 64); // every wave of the grid writes its partial (0 beyond the last row)
    CsrDotWs  ws    = {};
    if(dot)
    {
        RAMD_TRY(mat_dot_partials(m, grid, &ws.part1));
        ws.dotv  = dotv;
    }
    // gathers in flight per row: 8 where the rows average up to 8 off-diagonal entries (a 7-point operator has 6), else
    // k_csr_wr's 14
    const bool gw8 = m->nnz - m->nrow <= (int64_t)8 * m->nrow;
    with_mode_dot<false>(mode, dot, [&](auto M, auto D) {
        constexpr int  MODE = decltype(M)::value;
        constexpr bool DOT  = decltype(D)::value;
        if(gw8)
            hipLaunchKernelGGL((k_mcsr<T, MODE, DOT, 8>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->mcsr_ro, m->mcsr_ci,
                               (const T*)m->mcsr_val, x, y, scalar, ws);
        else
            hipLaunchKernelGGL((k_mcsr<T, MODE, DOT, 14>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->mcsr_ro, m->mcsr_ci,
                               (const T*)m->mcsr_val, x, y, scalar, ws);
    });
    RAMD_HIP(hipGetLastError());
    if(dot)
        return reduce_sum_to_slot(ws.part1, (int64_t)npart, slot);
    return RAMD_OK;
}
template int launch_mcsr<double>(const ramd_mat_s*, const double*, double*, int, double, bool, int, const double*);
template int launch_mcsr<float>(const ramd_mat_s*, const float*, float*, int, float, bool, int, const float*);

int mcsr_extract_diag(const ramd_mat_s* m, void* d, bool inv)
{
    Backend&  b    = backend();
    const int n    = m->nrow;
    const int grid = ew_grid(n);
    if(m->dtype == RAMD_F64 && inv)
        hipLaunchKernelGGL((k_mcsr_diag<double, true>), dim3(grid), dim3(kBlock), 0, b.cur, n, (const double*)m->mcsr_val, (double*)d);
    else if(m->dtype == RAMD_F64)
        hipLaunchKernelGGL((k_mcsr_diag<double, false>), dim3(grid), dim3(kBlock), 0, b.cur, n, (const double*)m->mcsr_val, (double*)d);
    else if(inv)
        hipLaunchKernelGGL((k_mcsr_diag<float, true>), dim3(grid), dim3(kBlock), 0, b.cur, n, (const float*)m->mcsr_val, (float*)d);
    else
        hipLaunchKernelGGL((k_mcsr_diag<float, false>), dim3(grid), dim3(kBlock), 0, b.cur, n, (const float*)m->mcsr_val, (float*)d);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

// ---------------------------------------------------------------------------------------------------- conversions (host side)
// the three arrays of an MCSR matrix with nnz entries on n rows; col[0 .. n) zero-filled (host_conversion.cpp:191-193)
static int mcsr_alloc(int dtype, int n, int64_t nnz, int** ro, int** ci, void** val)
{
    Backend& b = backend();
    int      s = dev_alloc(ro, (int64_t)n + 1);
    if(s == RAMD_OK)
        s = dev_alloc(ci, nnz);
    if(s == RAMD_OK && cached_malloc(val, (size_t)nnz * val_size(dtype) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && hipMemsetAsync(*ro, 0, sizeof(int) * ((size_t)n + 1), b.cur) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nnz > 0 && hipMemsetAsync(*ci, 0, sizeof(int) * (size_t)std::min<int64_t>(n, nnz), b.cur) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s != RAMD_OK)
    {
        dev_free(ro);
        dev_free(ci);
        if(*val)
            (void)cached_free(*val);
        *val = nullptr;
    }
    return s;
}

template <typename T>
static int csr_to_mcsr_t(ramd_mat_s* m)
{
    Backend&  b = backend();
    const int n = m->nrow;
    int *     ro = nullptr, *ci = nullptr;
    void*     val = nullptr;
    if(m->nnz > 0) // (a matrix without entries: an empty MCSR matrix, as the reference's ConvertFrom gives)
    {
        int* bad = nullptr;
        int  hb  = 0;
        RAMD_TRY(dev_alloc(&bad, 1));
        int s = hipMemsetAsync(bad, 0, sizeof(int), b.cur) == hipSuccess ? RAMD_OK : RAMD_ERR_HIP;
        if(s == RAMD_OK)
        {
            hipLaunchKernelGGL(k_mcsr_flag, dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, m->rp, m->ci, bad);
            if(hipGetLastError() != hipSuccess || hipMemcpyAsync(&hb, bad, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess)
                s = RAMD_ERR_HIP;
        }
        dev_free(&bad);
        RAMD_TRY(s);
        if(hb)
            RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_mcsr refused: a row does not store exactly one diagonal entry; matrix stays CSR");
    }
    RAMD_TRY(mcsr_alloc(m->dtype, n, m->nnz, &ro, &ci, &val));
    if(m->nnz > 0)
    {
        hipLaunchKernelGGL((k_mcsr_fill<T>), dim3(ew_grid((int64_t)n + 1)), dim3(kBlock), 0, b.cur, n, m->rp, m->ci, (const T*)m->val, ro,
                           ci, (T*)val);
        if(hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess)
        {
            dev_free(&ro);
            dev_free(&ci);
            (void)cached_free(val);
            RAMD_FAIL(RAMD_ERR_HIP, "csr_to_mcsr failed; the matrix stays CSR");
        }
    }
    const int64_t nnz = m->nnz;
    mat_free_csr(m);
    mat_free_analysis(m);
    m->mcsr_ro  = ro;
    m->mcsr_ci  = ci;
    m->mcsr_val = val;
    m->format   = RAMD_MCSR;
    m->nnz      = nnz;
    return RAMD_OK;
}

int csr_to_mcsr(ramd_mat_s* m)
{
    if(m->format != RAMD_CSR || mat_is_wide(m))
        RAMD_FAIL(RAMD_ERR_STATE, "csr_to_mcsr: the matrix is not a CSR matrix with 32-bit row offsets (internal)");
    if(m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_mcsr refused: MCSR holds square matrices only; matrix stays CSR");
    if(m->nnz > 0 && (!m->rp || !m->ci || !m->val))
        RAMD_FAIL(RAMD_ERR_STATE, "ConvertTo(MCSR): the matrix holds no CSR data");
    return m->dtype == RAMD_F64 ? csr_to_mcsr_t<double>(m) : csr_to_mcsr_t<float>(m);
}

template <typename T>
static int mcsr_to_csr_t(ramd_mat_s* m)
{
    Backend&      b   = backend();
    const int     n   = m->nrow;
    const int64_t nnz = m->nnz;
    int *         rp = nullptr, *ci = nullptr;
    void*         val = nullptr;
    int           s   = dev_alloc(&rp, (int64_t)n + 1);
    if(s == RAMD_OK)
        s = dev_alloc(&ci, nnz);
    if(s == RAMD_OK && cached_malloc(&val, (size_t)nnz * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nnz <= 0 && hipMemsetAsync(rp, 0, sizeof(int) * ((size_t)n + 1), b.cur) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nnz > 0)
        hipLaunchKernelGGL((k_mcsr2csr<T>), dim3(ew_grid((int64_t)n + 1)), dim3(kBlock), 0, b.cur, n, m->mcsr_ro, m->mcsr_ci,
                           (const T*)m->mcsr_val, rp, ci, (T*)val);
    if(s == RAMD_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess))
        s = RAMD_ERR_HIP;
    if(s != RAMD_OK)
    {
        dev_free(&rp);
        dev_free(&ci);
        if(val)
            (void)cached_free(val);
        RAMD_FAIL(s, "mcsr_to_csr failed; the matrix stays MCSR");
    }
    mat_free_mcsr(m);
    mat_free_analysis(m);
    m->rp     = rp;
    m->ci     = ci;
    m->val    = val;
    m->nnz    = nnz;
    m->format = RAMD_CSR;
    return RAMD_OK;
}

int mcsr_to_csr(ramd_mat_s* m)
{
    if(m->format != RAMD_MCSR || m->nrow != m->ncol || (m->nnz > 0 && (!m->mcsr_ro || !m->mcsr_ci || !m->mcsr_val)))
        RAMD_FAIL(RAMD_ERR_STATE, "mcsr_to_csr: the matrix holds no MCSR data");
    return m->dtype == RAMD_F64 ? mcsr_to_csr_t<double>(m) : mcsr_to_csr_t<float>(m);
}

} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_mat_set_mcsr(ramd_mat_t m, int nrow, int ncol, int64_t nnz, const int32_t* row_offset, const int32_t* col, const void* val)
{
    RAMD_NARROW_ONLY(m); // (a handle that holds 64-bit row offsets is cleared first, as every entry without a 64-bit path asks)
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(nrow < 0 || nrow != ncol || nnz < 0 || nnz > INT32_MAX || !row_offset || (nnz > 0 && (!col || !val)))
        RAMD_FAIL(RAMD_ERR_ARG, "bad MCSR arguments: a square matrix, its three arrays and at most INT32_MAX entries");
    if(row_offset[0] != nrow || row_offset[nrow] != nnz)
        RAMD_FAIL(RAMD_ERR_ARG, "bad MCSR arguments: row_offset[0] must be nrow and row_offset[nrow] nnz");
    for(int i = 0; i < nrow; ++i)
        if(row_offset[i + 1] < row_offset[i])
            RAMD_FAIL(RAMD_ERR_ARG, "bad MCSR arguments: the row offsets decrease");
    for(int64_t j = nrow; j < nnz; ++j)
        if(col[j] < 0 || col[j] >= ncol)
            RAMD_FAIL(RAMD_ERR_ARG, "bad MCSR arguments: a column outside [0, ncol)");
    int * ro = nullptr, *ci = nullptr;
    void* v  = nullptr;
    RAMD_TRY(mcsr_alloc(m->dtype, nrow, nnz, &ro, &ci, &v));
    Backend&   b = backend();
    hipError_t e = hipMemcpyAsync(ro, row_offset, sizeof(int) * ((size_t)nrow + 1), hipMemcpyHostToDevice, b.cur);
    if(e == hipSuccess && nnz > nrow) // (col[0 .. n) stays zero whatever the caller holds there)
        e = hipMemcpyAsync(ci + nrow, col + nrow, sizeof(int) * (size_t)(nnz - nrow), hipMemcpyHostToDevice, b.cur);
    if(e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(v, val, val_size(m->dtype) * (size_t)nnz, hipMemcpyHostToDevice, b.cur);
    if(e == hipSuccess)
        e = hipStreamSynchronize(b.cur);
    if(e != hipSuccess)
    {
        dev_free(&ro);
        dev_free(&ci);
        (void)cached_free(v);
        RAMD_HIP(e);
    }
    ramd_mat_clear(m);
    m->mcsr_ro  = ro;
    m->mcsr_ci  = ci;
    m->mcsr_val = v;
    m->format   = RAMD_MCSR;
    m->nrow = m->ncol = nrow;
    m->nnz            = nnz;
    return RAMD_OK;
}

int ramd_mat_copy_mcsr_to_host(ramd_mat_t m, int32_t* row_offset, int32_t* col, void* val)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format != RAMD_MCSR)
        RAMD_FAIL(RAMD_ERR_STATE, "matrix is not in MCSR format");
    Backend& b = backend();
    if(row_offset)
        RAMD_HIP(hipMemcpyAsync(row_offset, m->mcsr_ro, sizeof(int) * ((size_t)m->nrow + 1), hipMemcpyDeviceToHost, b.cur));
    if(col && m->nnz > 0)
        RAMD_HIP(hipMemcpyAsync(col, m->mcsr_ci, sizeof(int) * (size_t)m->nnz, hipMemcpyDeviceToHost, b.cur));
    if(val && m->nnz > 0)
        RAMD_HIP(hipMemcpyAsync(val, m->mcsr_val, val_size(m->dtype) * (size_t)m->nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));
    return RAMD_OK;
}

} // extern "C"
