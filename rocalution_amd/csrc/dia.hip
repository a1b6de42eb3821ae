// dia.hip -- the DIA format: CSR <-> DIA on the device and the diagonal-wise products.
//
// Replaces csr_to_dia / dia_to_csr (src/base/host/host_conversion.cpp:958-1113; the reference's HIP backend has kernels of its
// own, hip_conversion.cpp) and HostMatrixDIA::Apply / ApplyAdd (src/base/host/host_matrix_dia.cpp:300-420).  Layout: one slot
// per populated diagonal col - row, offsets ascending, values
//     DIA_IND(row, d, nrow, ndiag) = d * nrow + row                  (matrix_formats_ind.hpp:43-45)
// zero where CSR stores nothing.  Square matrices only (include/rocalution_amd.h has the reasons).
//
// The products.  A product reads no column index, no row offset and no pattern byte: per row 8 * ndiag bytes of values, x and y.
// One row per lane, 256 rows per workgroup: the 64 values a wave reads of one diagonal are contiguous, and so are the 64
// elements of x (a diagonal is a shifted copy of x's index range).  The offsets are the same for every lane, indexed by the
// loop counter alone, so they arrive by scalar loads -- no LDS table whose size ndiag could outgrow.  The diagonals are walked
// in chunks of kDiaU: all 2 * kDiaU loads of a chunk are issued before its first add; the adds keep the ascending order of
// the offsets, which is the order of the host loop, one rounded multiply and one rounded add per diagonal.  A workgroup whose
// 256 rows are interior for every diagonal (row_first + off[0] >= 0 and row_last + off[ndiag - 1] < n: the offsets ascend)
// runs without a range test; the others clamp the column of an out-of-range diagonal to element 0 and drop the product, so x
// is never read outside [0, n) and what lies at a clamped position never reaches a sum.
#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <climits>

namespace ramd
{

// ---------------------------------------------------------------------------------------------------- CSR -> DIA
// host_conversion.cpp:975-990: flag[col - row + n] = 1 for every stored entry (all writers store the same word)
__global__ __launch_bounds__(kBlock) void k_dia_flag(int n, const int* __restrict__ rp, const int* __restrict__ ci, int* __restrict__ flag)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz)
        for(int j = rp[row]; j < rp[row + 1]; ++j)
        {
            const int64_t k = (int64_t)ci[j] - row + n;
            if(k >= 0 && k < 2 * (int64_t)n) // (a column outside [0, n) names no diagonal of a square matrix)
                flag[k] = 1;
        }
}
// pos = exclusive scan of the 2 n + 1 flags: diagonal k - n is populated where pos[k + 1] > pos[k], and pos[k] is its slot
__global__ __launch_bounds__(kBlock) void k_dia_offsets(int n, const int* __restrict__ pos, int* __restrict__ off)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < 2 * (int64_t)n; k += gsz)
        if(pos[k + 1] > pos[k])
            off[pos[k]] = (int)(k - n);
}
// host_conversion.cpp:1020-1035: every entry to its slot (the values are zero before).  One thread walks a row front to back,
// so of two entries with the same column the later one stays, as there.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dia_fill(int n, const int* __restrict__ rp, const int* __restrict__ ci,
                                                     const T* __restrict__ val, const int* __restrict__ pos, T* __restrict__ dval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gsz)
        for(int j = rp[row]; j < rp[row + 1]; ++j)
        {
            const int64_t k = (int64_t)ci[j] - row + n;
            if(k >= 0 && k < 2 * (int64_t)n)
                dval[(int64_t)pos[k] * n + row] = val[j];
        }
}

// ---------------------------------------------------------------------------------------------------- DIA -> CSR
// host_conversion.cpp:1058-1107: a row keeps, diagonal after diagonal, the values that do not compare equal to zero (a padded
// zero, a stored zero and -0.0 go; NaN stays) whose column lies in [0, n).  FILL = false: counts (cnt[n] = 0 closes the scan)
template <typename T, bool FILL>
__global__ __launch_bounds__(kBlock) void k_dia2csr(int n, int ndiag, const int* __restrict__ off, const T* __restrict__ dval,
                                                    int* __restrict__ cnt, const int* __restrict__ rp, int* __restrict__ ci,
                                                    T* __restrict__ val)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row <= n; row += gsz)
    {
        int q = (FILL && row < n) ? rp[row] : 0;
        if(row < n)
            for(int d = 0; d < ndiag; ++d)
            {
                const int64_t c = row + off[d];
                if(c < 0 || c >= n)
                    continue;
                const T v = dval[(int64_t)d * n + row];
                if(v != (T)0)
                {
                    if(FILL)
                    {
                        ci[q]  = (int)c;
                        val[q] = v;
                    }
                    ++q;
                }
            }
        if(!FILL)
            cnt[row] = q;
    }
}

// ---------------------------------------------------------------------------------------------------- products
constexpr int kDiaU = 8; // diagonals of a chunk: 16 loads in flight per lane before the first add

template <typename T, int MODE>
__device__ __forceinline__ T dia_step(T acc, T a, T xv, T scalar)
{
    if(MODE == 1) // host_matrix_dia.cpp:409: out[i] += scalar * val * in
    {
        const T sa = scalar * a;
        const T t  = sa * xv;
        return acc + t;
    }
    const T t = a * xv;
    return acc + t;
}

// U diagonals from d on: the loads first, the adds in the order of the offsets.  `row` is a row of the matrix in every lane
// (the caller gives a lane beyond the last row row 0 and live = false)
template <typename T, int MODE, bool EDGE, int U>
__device__ __forceinline__ T dia_chunk(T acc, int d, int64_t n, int64_t row, bool live, const int* __restrict__ off,
                                       const T* __restrict__ val, const T* __restrict__ x, T scalar)
{
    T    a[U], b[U];
    bool ok[U];
#pragma unroll
    for(int u = 0; u < U; ++u)
    {
        const int64_t c = row + off[d + u];
        ok[u]           = !EDGE || (live && c >= 0 && c < n);
        b[u]            = x[ok[u] ? c : 0];
        a[u]            = nt_load(val + (int64_t)(d + u) * n + row);
    }
#pragma unroll
    for(int u = 0; u < U; ++u)
        if(ok[u])
            acc = dia_step<T, MODE>(acc, a[u], b[u], scalar);
    return acc;
}

template <typename T, int MODE, bool EDGE>
__device__ __forceinline__ T dia_row(T acc, int ndiag, int64_t n, int64_t row, bool live, const int* __restrict__ off,
                                     const T* __restrict__ val, const T* __restrict__ x, T scalar)
{
    int d = 0;
    for(; d + kDiaU <= ndiag; d += kDiaU)
        acc = dia_chunk<T, MODE, EDGE, kDiaU>(acc, d, n, row, live, off, val, x, scalar);
    switch(ndiag - d) // the rest as ONE chunk as well: a 7-point operator is all rest
    {
    case 7: return dia_chunk<T, MODE, EDGE, 7>(acc, d, n, row, live, off, val, x, scalar);
    case 6: return dia_chunk<T, MODE, EDGE, 6>(acc, d, n, row, live, off, val, x, scalar);
    case 5: return dia_chunk<T, MODE, EDGE, 5>(acc, d, n, row, live, off, val, x, scalar);
    case 4: return dia_chunk<T, MODE, EDGE, 4>(acc, d, n, row, live, off, val, x, scalar);
    case 3: return dia_chunk<T, MODE, EDGE, 3>(acc, d, n, row, live, off, val, x, scalar);
    case 2: return dia_chunk<T, MODE, EDGE, 2>(acc, d, n, row, live, off, val, x, scalar);
    case 1: return dia_chunk<T, MODE, EDGE, 1>(acc, d, n, row, live, off, val, x, scalar);
    default: return acc;
    }
}

// MODE 0: y = A x (DOT: and one partial of <dotv or x, y> per wave); MODE 1: y += (scalar * a) * x, diagonal by diagonal
template <typename T, int MODE, bool DOT>
__global__ __launch_bounds__(kBlock) void k_dia(int n, int ndiag, const int* __restrict__ off, const T* __restrict__ val,
                                                const T* __restrict__ x, T* __restrict__ y, T scalar, double* __restrict__ part1,
                                                const T* __restrict__ dotv)
{
    const int64_t row0 = (int64_t)blockIdx.x * kBlock;
    const int64_t rowt = row0 + threadIdx.x;
    const bool    live = rowt < n;
    const int64_t row  = live ? rowt : 0;
    T             acc  = (MODE == 1 && live) ? y[row] : (T)0;
    // (the same in every lane: the offsets ascend)
    const bool interior = row0 + kBlock <= n && row0 + off[0] >= 0 && row0 + (kBlock - 1) + off[ndiag - 1] < n;
    if(interior)
        acc = dia_row<T, MODE, false>(acc, ndiag, n, row, true, off, val, x, scalar);
    else
        acc = dia_row<T, MODE, true>(acc, ndiag, n, row, live, off, val, x, scalar);
    double dacc = 0.0;
    if(live)
    {
        nt_store(acc, y + row);
        if(DOT)
            dacc = (double)acc * (double)(dotv ? dotv[row] : x[row]);
    }
    if(DOT) // one partial per wave, added in their fixed order by reduce_sum_to_slot (as the CSR, ELL and BCSR kernels)
    {
        const double wsum = wave_reduce_sum(dacc);
        if((threadIdx.x & 63) == 0)
            part1[(int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)] = wsum;
    }
}

template <typename T>
int launch_dia(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv)
{
    Backend& b = backend();
    if(m->format != RAMD_DIA || m->nrow != m->ncol || m->nrow <= 0 || m->dia_ndiag <= 0 || !m->dia_off || !m->dia_val)
        RAMD_FAIL(RAMD_ERR_STATE, "DIA product: the matrix holds no DIA data (internal)");
    if(dot && mode != 0)
        RAMD_FAIL(RAMD_ERR_ARG, "DIA product: the fused dot goes with y = A x only (internal)");
    const int grid  = (int)(((int64_t)m->nrow + kBlock - 1) / kBlock);
    const int npart = grid * (kBlock / 64); // every wave of the grid writes its partial (0 beyond the last row)
    double*   part1 = nullptr;
    if(dot)
    {
        RAMD_TRY(mat_dot_partials(m, grid, &part1));
    }
    with_mode_dot<false>(mode, dot, [&](auto M, auto D) {
        hipLaunchKernelGGL((k_dia<T, decltype(M)::value, decltype(D)::value>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->dia_ndiag,
                           m->dia_off, (const T*)m->dia_val, x, y, scalar, part1, dotv);
    });
    RAMD_HIP(hipGetLastError());
    if(dot)
        return reduce_sum_to_slot(part1, (int64_t)npart, slot);
    return RAMD_OK;
}
template int launch_dia<double>(const ramd_mat_s*, const double*, double*, int, double, bool, int, const double*);
template int launch_dia<float>(const ramd_mat_s*, const float*, float*, int, float, bool, int, const float*);

// ---------------------------------------------------------------------------------------------------- conversions (host side)
template <typename T>
static int csr_to_dia_t(ramd_mat_s* m)
{
    Backend&      b  = backend();
    const int     n  = m->nrow;
    const int64_t nf = 2 * (int64_t)n + 1; // flags of the diagonals -n .. n - 1 (the first is never set), and the scan's total
    int *         pos = nullptr, *off = nullptr;
    void*         dv  = nullptr;
    int           nd  = 0;
    int           s   = RAMD_OK;
    if(n > 0 && m->nnz > 0) // (else: no diagonal, as the ELL path gives width 0)
    {
        RAMD_TRY(dev_alloc(&pos, nf));
        if(hipMemsetAsync(pos, 0, sizeof(int) * (size_t)nf, b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
        if(s == RAMD_OK)
        {
            hipLaunchKernelGGL(k_dia_flag, dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, m->rp, m->ci, pos);
            s = hipGetLastError() == hipSuccess ? device_exclusive_scan(pos, pos, nf) : RAMD_ERR_HIP;
        }
        if(s == RAMD_OK
           && (hipMemcpyAsync(&nd, pos + (nf - 1), sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess))
            s = RAMD_ERR_HIP;
        // host_conversion.cpp:993-997: "Conversion fails if DIA nnz exceeds 5 times CSR nnz" -- integer division
        if(s == RAMD_OK && nd > 5 * (m->nnz / n))
        {
            dev_free(&pos);
            RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_dia refused: num_diag > 5 * (nnz / nrow); matrix stays CSR");
        }
    }
    const int64_t nv = (int64_t)nd * n;
    if(s == RAMD_OK)
        s = dev_alloc(&off, nd);
    if(s == RAMD_OK && cached_malloc(&dv, (size_t)nv * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nv > 0)
    {
        hipError_t e = hipMemsetAsync(dv, 0, (size_t)nv * sizeof(T), b.cur);
        hipLaunchKernelGGL(k_dia_offsets, dim3(ew_grid(nf)), dim3(kBlock), 0, b.cur, n, pos, off);
        hipLaunchKernelGGL((k_dia_fill<T>), dim3(ew_grid(n)), dim3(kBlock), 0, b.cur, n, m->rp, m->ci, (const T*)m->val, pos, (T*)dv);
        if(e != hipSuccess || hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    dev_free(&pos);
    if(s != RAMD_OK)
    {
        dev_free(&off);
        if(dv)
            (void)cached_free(dv);
        RAMD_FAIL(s, "csr_to_dia failed; the matrix stays CSR");
    }
    mat_free_csr(m);
    mat_free_analysis(m);
    m->dia_off   = off;
    m->dia_val   = dv;
    m->dia_ndiag = nd;
    m->format    = RAMD_DIA;
    m->nnz       = nv;
    return RAMD_OK;
}

int csr_to_dia(ramd_mat_s* m)
{
    if(m->format != RAMD_CSR || mat_is_wide(m))
        RAMD_FAIL(RAMD_ERR_STATE, "csr_to_dia: the matrix is not a CSR matrix with 32-bit row offsets (internal)");
    if(m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_dia refused: DIA is provided for square matrices only; matrix stays CSR");
    if(m->nrow > 0 && m->nnz > 0 && !m->rp)
        RAMD_FAIL(RAMD_ERR_STATE, "ConvertTo(DIA): the matrix holds no CSR data");
    return m->dtype == RAMD_F64 ? csr_to_dia_t<double>(m) : csr_to_dia_t<float>(m);
}

template <typename T>
static int dia_to_csr_t(ramd_mat_s* m)
{
    Backend&  b  = backend();
    const int n  = m->nrow, nd = m->dia_ndiag;
    if(m->nnz > INT32_MAX)
        RAMD_FAIL(RAMD_ERR_UNSUPPORTED, "dia_to_csr: not provided for more than INT32_MAX DIA values; the matrix stays DIA");
    int * rp = nullptr, *ci = nullptr;
    void* val = nullptr;
    int   nnz = 0;
    RAMD_TRY(dev_alloc(&rp, (int64_t)n + 1));
    const int grid = ew_grid((int64_t)n + 1);
    hipLaunchKernelGGL((k_dia2csr<T, false>), dim3(grid), dim3(kBlock), 0, b.cur, n, nd, m->dia_off, (const T*)m->dia_val, rp,
                       (const int*)nullptr, (int*)nullptr, (T*)nullptr);
    int s = hipGetLastError() == hipSuccess ? device_exclusive_scan(rp, rp, (int64_t)n + 1) : RAMD_ERR_HIP;
    if(s == RAMD_OK
       && (hipMemcpyAsync(&nnz, rp + n, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
           || hipStreamSynchronize(b.cur) != hipSuccess))
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK)
        s = dev_alloc(&ci, nnz);
    if(s == RAMD_OK && cached_malloc(&val, (size_t)nnz * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK && nnz > 0)
    {
        hipLaunchKernelGGL((k_dia2csr<T, true>), dim3(grid), dim3(kBlock), 0, b.cur, n, nd, m->dia_off, (const T*)m->dia_val,
                           (int*)nullptr, (const int*)rp, ci, (T*)val);
        if(hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    if(s != RAMD_OK)
    {
        dev_free(&rp);
        dev_free(&ci);
        if(val)
            (void)cached_free(val);
        RAMD_FAIL(s, "dia_to_csr failed; the matrix stays DIA");
    }
    mat_free_dia(m);
    mat_free_analysis(m);
    m->rp     = rp;
    m->ci     = ci;
    m->val    = val;
    m->nnz    = nnz;
    m->format = RAMD_CSR;
    return RAMD_OK;
}

int dia_to_csr(ramd_mat_s* m)
{
    if(m->format != RAMD_DIA || (m->dia_ndiag > 0 && (!m->dia_off || !m->dia_val)))
        RAMD_FAIL(RAMD_ERR_STATE, "dia_to_csr: the matrix holds no DIA data");
    return m->dtype == RAMD_F64 ? dia_to_csr_t<double>(m) : dia_to_csr_t<float>(m);
}

} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_mat_dia_info(ramd_mat_t m, int* num_diag)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format != RAMD_DIA)
        RAMD_FAIL(RAMD_ERR_STATE, "matrix is not in DIA format");
    if(num_diag)
        *num_diag = m->dia_ndiag;
    return RAMD_OK;
}

int ramd_mat_copy_dia_to_host(ramd_mat_t m, int32_t* offset, void* val)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format != RAMD_DIA)
        RAMD_FAIL(RAMD_ERR_STATE, "matrix is not in DIA format");
    Backend& b = backend();
    if(offset && m->dia_ndiag > 0)
        RAMD_HIP(hipMemcpyAsync(offset, m->dia_off, sizeof(int) * (size_t)m->dia_ndiag, hipMemcpyDeviceToHost, b.cur));
    if(val && m->nnz > 0)
        RAMD_HIP(hipMemcpyAsync(val, m->dia_val, val_size(m->dtype) * (size_t)m->nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));
    return RAMD_OK;
}

} // extern "C"
