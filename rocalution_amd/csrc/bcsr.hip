// bcsr.hip -- the BCSR format: CSR <-> BCSR on the device and the block-row products.
//
// Replaces csr_to_bcsr / bcsr_to_csr (src/base/host/host_conversion.cpp:326-579; the reference's HIP backend calls
// rocsparse_csr2bsr) and HostMatrixBCSR::Apply / ApplyAdd (src/base/host/host_matrix_bcsr.cpp:330-429; rocsparse_bsrmv on
// its HIP backend).  Layout: square blocks of `dim`, column-major inside a block,
//     BCSR_IND(j, bi, bj, dim) = j * dim * dim + bi + bj * dim      (matrix_formats_ind.hpp:48)
// block columns distinct and ascending inside a block row, zero where CSR stores nothing.
//
// The products.  One block's dim^2 values are contiguous and so are the blocks of a block row and the block rows of a wave:
// a wave owns G = 64 / dim consecutive block rows (lane = one output row, 60 of 64 lanes at dim 5), and the values of ALL its
// block rows are ONE contiguous range.  The wave streams that range in steps of CH blocks through an LDS image of its own with
// 16-byte loads (the range start rounded down to a packet), stages the dim elements of x of every block column of the step
// beside it -- read once, shared by the dim rows of the block row -- and every lane then walks the blocks of ITS block row
// that the step holds: blocks in stored order, bj = 0 .. dim - 1, one rounded multiply and one rounded add per stored value,
// from 0, as the host loop does.  A block row longer than a step simply continues in the next one.  No workgroup barrier:
// the image is the wave's (wave_rows.hpp has the measurements behind that choice).  dim is a template parameter for 2 .. 5;
// every other dim runs k_bcsr_any, one lane per output row straight from memory: the lanes of a block row read dim
// consecutive values per step (a block column of the block), so a wave's load is 64 / dim pieces of dim values -- no LDS is
// sized by dim there, dim == nrow is served.
#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <climits>

namespace ramd
{

// ---------------------------------------------------------------------------------------------------- CSR -> BCSR
// The block columns of a block row, ascending: one wave per block row finds, turn by turn, the smallest block column above the
// last one among the entries of its dim rows (which are one contiguous range of the CSR arrays).  No order of the columns
// inside a CSR row is assumed.  FILL = false: counts (cnt[nrowb] = 0 closes the scan); FILL = true: writes them at brp[bi].
template <bool FILL>
__global__ __launch_bounds__(kBlock) void k_bcsr_cols(int nrowb, int dim, const int* __restrict__ rp, const int* __restrict__ ci,
                                                      int* __restrict__ cnt, const int* __restrict__ brp, int* __restrict__ bci)
{
    const int     lane = threadIdx.x & 63;
    const int64_t nw   = (int64_t)gridDim.x * (kBlock / 64);
    for(int64_t bi = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); bi < nrowb; bi += nw)
    {
        const int e0 = rp[bi * dim], e1 = rp[(bi + 1) * dim];
        const int base = FILL ? brp[bi] : 0;
        int       last = -1, n = 0;
        for(;;)
        {
            int mn = INT_MAX;
            for(int j = e0 + lane; j < e1; j += 64)
            {
                const int bc = ci[j] / dim;
                if(bc > last && bc < mn)
                    mn = bc;
            }
#pragma unroll
            for(int off = 32; off > 0; off >>= 1)
            {
                const int o = __shfl_xor(mn, off, 64);
                mn          = o < mn ? o : mn;
            }
            if(mn == INT_MAX) // (the same in every lane)
                break;
            if(FILL && lane == 0)
                bci[base + n] = mn;
            last = mn;
            ++n;
        }
        if(!FILL && lane == 0)
            cnt[bi] = n;
    }
    if(!FILL && blockIdx.x == 0 && threadIdx.x == 0)
        cnt[nrowb] = 0;
}

// host_conversion.cpp:453-490: every CSR entry goes to its place in its block (the values are zero before).  One thread walks
// a row front to back, so of two entries with the same column the later one stays, as there.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bcsr_vals(int nrow, int dim, const int* __restrict__ rp, const int* __restrict__ ci,
                                                      const T* __restrict__ val, const int* __restrict__ brp,
                                                      const int* __restrict__ bci, T* __restrict__ bval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < nrow; row += gsz)
    {
        const int bi = (int)(row / dim), i = (int)(row - (int64_t)bi * dim);
        const int b0 = brp[bi], b1 = brp[bi + 1];
        for(int j = rp[row]; j < rp[row + 1]; ++j)
        {
            const int c = ci[j], bc = c / dim, jj = c - bc * dim;
            int       lo = b0, hi = b1; // first k in [b0, b1) with bci[k] >= bc
            while(lo < hi)
            {
                const int mid = lo + (hi - lo) / 2;
                if(bci[mid] < bc)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if(lo < b1 && bci[lo] == bc && jj >= 0)
                bval[(int64_t)lo * dim * dim + i + (int64_t)jj * dim] = val[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- BCSR -> CSR
// host_conversion.cpp:537-579: row i * dim + r holds, block after block, the dim entries of line r of every block of block row
// i -- all of them, padded zeros included; columns ascending because the block columns are
template <typename T>
__global__ __launch_bounds__(kBlock) void k_bcsr2csr(int nrow, int dim, const int* __restrict__ brp, const int* __restrict__ bci,
                                                     const T* __restrict__ bval, int* __restrict__ rp, int* __restrict__ ci,
                                                     T* __restrict__ val)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < nrow; row += gsz)
    {
        const int     bi = (int)(row / dim), r = (int)(row - (int64_t)bi * dim);
        const int     b0 = brp[bi], b1 = brp[bi + 1];
        const int64_t p0 = (int64_t)b0 * dim * dim + (int64_t)r * (b1 - b0) * dim;
        rp[row]          = (int)p0;
        if(row == nrow - 1)
            rp[nrow] = (int)(p0 + (int64_t)(b1 - b0) * dim);
        int64_t p = p0;
        for(int k = b0; k < b1; ++k)
        {
            const int bc = bci[k];
            for(int c = 0; c < dim; ++c, ++p)
            {
                ci[p]  = dim * bc + c;
                val[p] = bval[(int64_t)k * dim * dim + r + (int64_t)c * dim];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- products
template <int D>
struct BcsrGeom
{
    static constexpr int G  = 64 / D; // block rows of a wave
    static constexpr int CH = D <= 2 ? 128 : (D <= 3 ? 64 : 32); // blocks of a step: at most 800 values + 160 elements of x per wave
};

template <typename T, int MODE, bool DOT>
__device__ __forceinline__ void bcsr_row_epilogue(bool live, int64_t wave, int64_t row, T sum, T* __restrict__ y, T scalar,
                                                  const T* __restrict__ x, const T* __restrict__ dotv, double* __restrict__ part1)
{
    double dacc = 0.0;
    if(live)
    {
        if(MODE == 1) // host_matrix_bcsr.cpp:425: out += scalar * sum
        {
            const T t = scalar * sum;
            sum       = y[row] + t;
        }
        nt_store(sum, y + row);
        if(DOT)
            dacc = (double)sum * (double)(dotv ? dotv[row] : x[row]);
    }
    if(DOT) // one partial per wave, added in their fixed order by reduce_sum_to_slot (as the CSR and ELL kernels)
    {
        const double wsum = wave_reduce_sum(dacc);
        if((threadIdx.x & 63) == 0)
            part1[wave] = wsum;
    }
}

template <typename T, int D, int MODE, bool DOT>
__global__ __launch_bounds__(kBlock) void k_bcsr(int nrowb, const int* __restrict__ brp, const int* __restrict__ bci,
                                                 const T* __restrict__ bval, const T* __restrict__ x, T* __restrict__ y, T scalar,
                                                 double* __restrict__ part1, const T* __restrict__ dotv)
{
    using VP          = typename Pack<T>::type;
    constexpr int VN  = Pack<T>::N;
    constexpr int G   = BcsrGeom<D>::G;
    constexpr int CH  = BcsrGeom<D>::CH;
    constexpr int DD  = D * D;
    constexpr int SVN = (CH * DD + VN + VN - 1) / VN * VN; // a step's values, the slack of the packet its first one starts in
    __shared__ __attribute__((aligned(16))) T sval[kBlock / 64][SVN];
    __shared__ T                              sxv[kBlock / 64][CH * D];
    const int     w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + w;
    const int64_t i0   = wave * G; // the wave's first block row
    const int     g = lane / D, bi = lane - g * D;
    const bool    live = g < G && i0 + g < nrowb;
    T*            sv   = sval[w];
    T*            sx   = sxv[w];
    T             sum  = (T)0;
    if(i0 < nrowb) // (the same in every lane of the wave)
    {
        const int64_t iend = i0 + G < nrowb ? i0 + G : nrowb;
        const int     B0 = brp[i0], B1 = brp[iend];
        const int     kb = live ? brp[i0 + g] : 0, ke = live ? brp[i0 + g + 1] : 0;
        for(int c0 = B0; c0 < B1; c0 += CH)
        {
            const int     n  = B1 - c0 < CH ? B1 - c0 : CH;
            const int64_t e0 = (int64_t)c0 * DD, ea = e0 & ~(int64_t)(VN - 1);
            const int     sh = (int)(e0 - ea); // where the step's first value lies in the image
            const int     npk = (sh + n * DD + VN - 1) / VN; // <= SVN / VN; the last packet may run past the array's end: kPad
            const VP*     src = reinterpret_cast<const VP*>(bval + ea);
            for(int p = lane; p < npk; p += 64)
                *reinterpret_cast<VP*>(sv + p * VN) = nt_load(src + p);
            for(int idx = lane; idx < n * D; idx += 64) // x once per block column: dim contiguous elements
            {
                const int b = idx / D, bj = idx - b * D;
                sx[idx]     = x[(int64_t)D * bci[c0 + b] + bj];
            }
            __builtin_amdgcn_wave_barrier();
            const int lo = kb > c0 ? kb : c0, hi = ke < c0 + n ? ke : c0 + n;
            for(int k = lo; k < hi; ++k) // the lane's blocks of this step, in stored order
            {
                const T* a  = sv + sh + (k - c0) * DD + bi;
                const T* xv = sx + (k - c0) * D;
#pragma unroll
                for(int bj = 0; bj < D; ++bj)
                    sum += a[bj * D] * xv[bj];
            }
            __builtin_amdgcn_wave_barrier(); // (the next step overwrites the image)
        }
    }
    bcsr_row_epilogue<T, MODE, DOT>(live, wave, (i0 + g) * D + bi, sum, y, scalar, x, dotv, part1);
}

// any dim: one lane per output row
template <typename T, int MODE, bool DOT>
__global__ __launch_bounds__(kBlock) void k_bcsr_any(int nrow, int dim, const int* __restrict__ brp, const int* __restrict__ bci,
                                                     const T* __restrict__ bval, const T* __restrict__ x, T* __restrict__ y,
                                                     T scalar, double* __restrict__ part1, const T* __restrict__ dotv)
{
    const int64_t row  = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool    live = row < nrow;
    T             sum  = (T)0;
    if(live)
    {
        const int     ai = (int)(row / dim), bi = (int)(row - (int64_t)ai * dim);
        const int     b0 = brp[ai], b1 = brp[ai + 1];
        const int64_t dd = (int64_t)dim * dim;
        for(int aj = b0; aj < b1; ++aj)
        {
            const T* a  = bval + aj * dd + bi;
            const T* xv = x + (int64_t)dim * bci[aj];
            for(int bj = 0; bj < dim; ++bj)
                sum += a[(int64_t)bj * dim] * xv[bj];
        }
    }
    bcsr_row_epilogue<T, MODE, DOT>(live, (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), row, sum, y, scalar, x, dotv,
                                    part1);
}

template <typename T>
int launch_bcsr(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv)
{
    Backend&  b   = backend();
    const int dim = m->bcsr_dim;
    if(m->format != RAMD_BCSR || dim < 2 || !m->bcsr_rp || m->bcsr_nrowb <= 0)
        RAMD_FAIL(RAMD_ERR_STATE, "BCSR product: the matrix holds no BCSR data (internal)");
    if(dot && mode != 0)
        RAMD_FAIL(RAMD_ERR_ARG, "BCSR product: the fused dot goes with y = A x only (internal)");
    const bool    fixed = dim <= 5;
    const int     g     = fixed ? 64 / dim : 0;
    const int64_t nwave = fixed ? ((int64_t)m->bcsr_nrowb + g - 1) / g : ((int64_t)m->nrow + 63) / 64;
    const int     grid  = (int)((nwave + kBlock / 64 - 1) / (kBlock / 64));
    const int     npart = grid * (kBlock / 64); // every wave of the grid writes its partial (0 beyond the last row)
    double*       part1 = nullptr;
    if(dot)
    {
        RAMD_TRY(mat_dot_partials(m, grid, &part1));
    }
    with_mode_dot<false>(mode, dot, [&](auto M, auto D) {
        constexpr int  MODE = decltype(M)::value;
        constexpr bool DOT  = decltype(D)::value;
        auto fixed_dim = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, b.cur, m->bcsr_nrowb, m->bcsr_rp, m->bcsr_ci, (const T*)m->bcsr_val, x,
                               y, scalar, part1, dotv);
        };
        if(dim == 2)
            fixed_dim(k_bcsr<T, 2, MODE, DOT>);
        else if(dim == 3)
            fixed_dim(k_bcsr<T, 3, MODE, DOT>);
        else if(dim == 4)
            fixed_dim(k_bcsr<T, 4, MODE, DOT>);
        else if(dim == 5)
            fixed_dim(k_bcsr<T, 5, MODE, DOT>);
        else
            hipLaunchKernelGGL((k_bcsr_any<T, MODE, DOT>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, dim, m->bcsr_rp, m->bcsr_ci,
                               (const T*)m->bcsr_val, x, y, scalar, part1, dotv);
    });
    RAMD_HIP(hipGetLastError());
    if(dot)
        return reduce_sum_to_slot(part1, (int64_t)npart, slot);
    return RAMD_OK;
}
template int launch_bcsr<double>(const ramd_mat_s*, const double*, double*, int, double, bool, int, const double*);
template int launch_bcsr<float>(const ramd_mat_s*, const float*, float*, int, float, bool, int, const float*);

// ---------------------------------------------------------------------------------------------------- conversions (host side)
template <typename T>
static int csr_to_bcsr(ramd_mat_s* m, int dim)
{
    Backend&      b     = backend();
    const int     nrowb = m->nrow / dim, ncolb = m->ncol / dim;
    const int64_t nwv   = std::max(nrowb, 1);
    const int     wgrid = (int)std::min<int64_t>((nwv + kBlock / 64 - 1) / (kBlock / 64), (int64_t)b.num_cu * 64);
    int *         brp = nullptr, *bci = nullptr;
    void*         bv  = nullptr;
    RAMD_TRY(dev_alloc(&brp, (int64_t)nrowb + 1));
    hipLaunchKernelGGL((k_bcsr_cols<false>), dim3(wgrid), dim3(kBlock), 0, b.cur, nrowb, dim, m->rp, m->ci, brp, (const int*)nullptr,
                       (int*)nullptr);
    int s    = hipGetLastError() == hipSuccess ? device_exclusive_scan(brp, brp, (int64_t)nrowb + 1) : RAMD_ERR_HIP;
    int nnzb = 0;
    if(s == RAMD_OK
       && (hipMemcpyAsync(&nnzb, brp + nrowb, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
           || hipStreamSynchronize(b.cur) != hipSuccess))
        s = RAMD_ERR_HIP;
    const int64_t nv = (int64_t)nnzb * dim * dim;
    if(s == RAMD_OK && nv > INT32_MAX)
    {
        set_error(__FILE__, __LINE__, "csr_to_bcsr: more than INT32_MAX values with the blocks filled");
        s = RAMD_ERR_UNSUPPORTED;
    }
    if(s == RAMD_OK)
        s = dev_alloc(&bci, nnzb);
    if(s == RAMD_OK && cached_malloc(&bv, (size_t)nv * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nnzb > 0)
    {
        hipError_t e = hipMemsetAsync(bv, 0, (size_t)nv * sizeof(T), b.cur);
        hipLaunchKernelGGL((k_bcsr_cols<true>), dim3(wgrid), dim3(kBlock), 0, b.cur, nrowb, dim, m->rp, m->ci, (int*)nullptr, brp, bci);
        hipLaunchKernelGGL((k_bcsr_vals<T>), dim3(ew_grid(m->nrow)), dim3(kBlock), 0, b.cur, m->nrow, dim, m->rp, m->ci,
                           (const T*)m->val, brp, bci, (T*)bv);
        if(e != hipSuccess || hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    if(s != RAMD_OK)
    {
        dev_free(&brp);
        dev_free(&bci);
        if(bv)
            (void)cached_free(bv);
        return s; // (the matrix is CSR as before)
    }
    mat_free_csr(m);
    mat_free_analysis(m);
    m->bcsr_rp    = brp;
    m->bcsr_ci    = bci;
    m->bcsr_val   = bv;
    m->bcsr_dim   = dim;
    m->bcsr_nrowb = nrowb;
    m->bcsr_ncolb = ncolb;
    m->bcsr_nnzb  = nnzb;
    m->format     = RAMD_BCSR;
    m->nnz        = nv;
    return RAMD_OK;
}

template <typename T>
static int bcsr_to_csr_t(ramd_mat_s* m)
{
    Backend&      b   = backend();
    const int64_t nnz = m->nnz; // nnzb * dim^2 <= INT32_MAX
    int *         rp = nullptr, *ci = nullptr;
    void*         val = nullptr;
    RAMD_TRY(dev_alloc(&rp, (int64_t)m->nrow + 1));
    int s = dev_alloc(&ci, nnz);
    if(s == RAMD_OK && cached_malloc(&val, (size_t)nnz * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK)
    {
        if(m->nrow > 0)
            hipLaunchKernelGGL((k_bcsr2csr<T>), dim3(ew_grid(m->nrow)), dim3(kBlock), 0, b.cur, m->nrow, m->bcsr_dim, m->bcsr_rp,
                               m->bcsr_ci, (const T*)m->bcsr_val, rp, ci, (T*)val);
        else if(hipMemsetAsync(rp, 0, sizeof(int), b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
        if(hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    if(s != RAMD_OK)
    {
        dev_free(&rp);
        dev_free(&ci);
        if(val)
            (void)cached_free(val);
        RAMD_FAIL(s, "bcsr_to_csr failed; the matrix stays BCSR");
    }
    mat_free_bcsr(m);
    mat_free_analysis(m);
    m->rp     = rp;
    m->ci     = ci;
    m->val    = val;
    m->nnz    = nnz;
    m->format = RAMD_CSR;
    return RAMD_OK;
}

int bcsr_to_csr(ramd_mat_s* m)
{
    if(m->format != RAMD_BCSR || !m->bcsr_rp)
        RAMD_FAIL(RAMD_ERR_STATE, "bcsr_to_csr: the matrix holds no BCSR data");
    return m->dtype == RAMD_F64 ? bcsr_to_csr_t<double>(m) : bcsr_to_csr_t<float>(m);
}

} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_mat_convert_bcsr(ramd_mat_t m, int blockdim)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(blockdim < 2)
        RAMD_FAIL(RAMD_ERR_ARG, "ConvertTo(BCSR): the block dimension must be 2 or more");
    if(m->format == RAMD_BCSR) // local_matrix.cpp:2075: nothing to do for a matrix in the target format, whatever its blockdim
        return RAMD_OK;
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED; // X -> CSR -> BCSR goes through the caller
    if(!m->rp) // (never allocated)
        RAMD_FAIL(RAMD_ERR_STATE, "ConvertTo(BCSR): the matrix holds no CSR data");
    if(m->nrow % blockdim != 0 || m->ncol % blockdim != 0) // host_conversion.cpp:342-345
        RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_bcsr refused: nrow and ncol must be multiples of blockdim; matrix stays CSR");
    return m->dtype == RAMD_F64 ? csr_to_bcsr<double>(m, blockdim) : csr_to_bcsr<float>(m, blockdim);
}

int ramd_mat_bcsr_info(ramd_mat_t m, int* blockdim, int* nrowb, int* ncolb, int64_t* nnzb)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format != RAMD_BCSR)
        RAMD_FAIL(RAMD_ERR_STATE, "matrix is not in BCSR format");
    if(blockdim)
        *blockdim = m->bcsr_dim;
    if(nrowb)
        *nrowb = m->bcsr_nrowb;
    if(ncolb)
        *ncolb = m->bcsr_ncolb;
    if(nnzb)
        *nnzb = m->bcsr_nnzb;
    return RAMD_OK;
}

int ramd_mat_copy_bcsr_to_host(ramd_mat_t m, int32_t* row_offset, int32_t* col, void* val)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format != RAMD_BCSR)
        RAMD_FAIL(RAMD_ERR_STATE, "matrix is not in BCSR format");
    Backend& b = backend();
    if(row_offset)
        RAMD_HIP(hipMemcpyAsync(row_offset, m->bcsr_rp, sizeof(int) * ((size_t)m->bcsr_nrowb + 1), hipMemcpyDeviceToHost, b.cur));
    if(col && m->bcsr_nnzb > 0)
        RAMD_HIP(hipMemcpyAsync(col, m->bcsr_ci, sizeof(int) * (size_t)m->bcsr_nnzb, hipMemcpyDeviceToHost, b.cur));
    if(val && m->nnz > 0)
        RAMD_HIP(hipMemcpyAsync(val, m->bcsr_val, val_size(m->dtype) * (size_t)m->nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));
    return RAMD_OK;
}

} // extern "C"
