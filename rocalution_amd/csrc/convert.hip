// convert.hip -- format conversion, value cast, sub-matrix extraction, P A P^T (setup-time kernels).
//
// Replaces src/base/hip/hip_conversion.cpp (rocsparse_csr2ell, custom csr2hyb + rocPRIM scan),
// and the Permute / ExtractSubMatrix kernels of src/base/hip/hip_matrix_csr.cpp:962-1190, :3374-3478.
// Layout RULES are the reference's (src/base/host/host_conversion.cpp, cited per function): the
// resulting arrays are identical to the host backend's, entry for entry.
#include "csr_filter.hpp"
#include "device_utils.hpp"
#include "matrix_impl.hpp"

namespace ramd
{

__global__ __launch_bounds__(kBlock) void k_row_nnz(int nrow, const int* __restrict__ rp,
                                                    int* __restrict__ out, int minus, int clamp0)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        int v = rp[i + 1] - rp[i] - minus;
        out[i] = (clamp0 && v < 0) ? 0 : v;
    }
}

// host_conversion.cpp:658-684: fill ELL (column-major), pad col=-1 val=0
template <typename T>
__global__ __launch_bounds__(kBlock) void k_csr2ell(int nrow, int width, const int* __restrict__ rp,
                                                    const int* __restrict__ ci,
                                                    const T* __restrict__ val,
                                                    int* __restrict__ ecol, T* __restrict__ eval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        int n = 0;
        for(int j = rp[i]; j < rp[i + 1]; ++j, ++n)
        {
            ecol[(int64_t)n * nrow + i] = ci[j];
            eval[(int64_t)n * nrow + i] = val[j];
        }
        for(; n < width; ++n)
        {
            ecol[(int64_t)n * nrow + i] = -1;
            eval[(int64_t)n * nrow + i] = (T)0;
        }
    }
}

// host_conversion.cpp:1199-1234: first `width` entries of a row -> ELL, the rest -> COO
template <typename T>
__global__ __launch_bounds__(kBlock) void k_csr2hyb(int nrow, int width, const int* __restrict__ rp,
                                                    const int* __restrict__ ci,
                                                    const T* __restrict__ val,
                                                    const int* __restrict__ coo_rp,
                                                    int* __restrict__ ecol, T* __restrict__ eval,
                                                    int* __restrict__ crow, int* __restrict__ ccol,
                                                    T* __restrict__ cval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        int p = 0;
        int c = coo_rp[i];
        for(int j = rp[i]; j < rp[i + 1]; ++j)
        {
            if(p < width)
            {
                ecol[(int64_t)p * nrow + i] = ci[j];
                eval[(int64_t)p * nrow + i] = val[j];
                ++p;
            }
            else
            {
                crow[c] = (int)i;
                ccol[c] = ci[j];
                cval[c] = val[j];
                ++c;
            }
        }
        for(; p < width; ++p)
        {
            ecol[(int64_t)p * nrow + i] = -1;
            eval[(int64_t)p * nrow + i] = (T)0;
        }
    }
}

// host_conversion.cpp:596-610: COO row index expansion
__global__ __launch_bounds__(kBlock) void k_expand_rows(int nrow, const int* __restrict__ rp,
                                                        int* __restrict__ crow)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
        for(int j = rp[i]; j < rp[i + 1]; ++j)
            crow[j] = (int)i;
}

// compaction of the non-empty rows of a row-pointer array: grow[k] = row, gptr[k] = rp[row]
__global__ __launch_bounds__(kBlock) void k_compact_rows(int nrow, const int* __restrict__ rp,
                                                         const int* __restrict__ pos,
                                                         int* __restrict__ grow,
                                                         int* __restrict__ gptr)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
        if(rp[i + 1] > rp[i])
        {
            grow[pos[i]] = (int)i;
            gptr[pos[i]] = rp[i];
        }
}

__global__ __launch_bounds__(kBlock) void k_flag_nonempty(int nrow, const int* __restrict__ rp,
                                                          int* __restrict__ flag)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nrow; i += gsz)
        flag[i] = (i < nrow && rp[i + 1] > rp[i]) ? 1 : 0;
}

template <typename D, typename S>
__global__ __launch_bounds__(kBlock) void k_cast_vals(int64_t n, D* dst, const S* src)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gsz)
        dst[i] = static_cast<D>(src[i]);
}

// ---- sub-matrix extraction: host_matrix_csr.cpp:848-916, as a rule of csr_filter.hpp (the source may be wide, the result
// is narrow: it has to fit)
struct SubRule
{
    static constexpr bool kRowsOnce = true;
    int                   r0, c0, cs;
    __device__ FilterRow row(int64_t i) const { return FilterRow{r0 + (int)i}; }
    template <typename T>
    __device__ bool keep(const FilterRow&, int col, T) const { return col >= c0 && col < c0 + cs; }
    __device__ int  col(const FilterRow&, int col) const { return col - c0; }
};

// ---- P A P^T: host_matrix_csr.cpp:3848-3958 (row i -> perm[i]; col -> perm[col]; columns of each
// row sorted ascending by insertion -- entries are unique, so the result equals the reference's)
__global__ __launch_bounds__(kBlock) void k_perm_row_nnz(int nrow, const int* __restrict__ rp,
                                                         const int* __restrict__ perm,
                                                         int* __restrict__ out)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nrow; i += gsz)
    {
        if(i < nrow)
            out[perm[i]] = rp[i + 1] - rp[i];
        else
            out[nrow] = 0;
    }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_perm_fill(int nrow, const int* __restrict__ rp,
                                                      const int* __restrict__ ci,
                                                      const T* __restrict__ val,
                                                      const int* __restrict__ perm,
                                                      const int* __restrict__ orp,
                                                      int* __restrict__ oci, T* __restrict__ oval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        const int base = orp[perm[i]];
        const int src  = rp[i];
        const int rn   = rp[i + 1] - src;
        for(int j = 0; j < rn; ++j)
        {
            const int comp = perm[ci[src + j]];
            const T   v    = val[src + j];
            int       k    = j - 1;
            for(; k >= 0; --k)
            {
                if(oci[base + k] > comp)
                {
                    oci[base + k + 1]  = oci[base + k];
                    oval[base + k + 1] = oval[base + k];
                }
                else
                    break;
            }
            oci[base + k + 1]  = comp;
            oval[base + k + 1] = v;
        }
    }
}

// ---- X -> CSR (host_conversion.cpp:690-760 ell_to_csr, :765-880 hyb_to_csr, :884-960 coo_to_csr):
// a row keeps its valid ELL entries (0 <= col < ncol) in slot order, then its COO entries in storage
// order; plain COO additionally gets its columns sorted inside every row (stable, as the bubble sort).
__global__ __launch_bounds__(kBlock) void k_x2csr_count_ell(int nrow, int ncol, int width,
                                                            const int* __restrict__ ecol,
                                                            int* __restrict__ cnt)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= nrow; t += gsz)
    {
        int c = 0;
        if(t < nrow)
            for(int el = 0; el < width; ++el)
            {
                const int col = ecol[(int64_t)el * nrow + t];
                if(col >= 0 && col < ncol)
                    ++c;
            }
        cnt[t] = c;
    }
}
__global__ __launch_bounds__(kBlock) void k_x2csr_count_coo(int ngroups, const int* __restrict__ grow,
                                                            const int* __restrict__ gptr,
                                                            int* __restrict__ cnt)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gsz)
        cnt[grow[g]] += gptr[g + 1] - gptr[g]; // a row is in at most one group
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_x2csr_fill_ell(int nrow, int ncol, int width,
                                                           const int* __restrict__ ecol,
                                                           const T* __restrict__ eval,
                                                           const int* __restrict__ rp,
                                                           int* __restrict__ oci, T* __restrict__ oval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nrow; t += gsz)
    {
        int ind = rp[t];
        for(int el = 0; el < width; ++el)
        {
            const int col = ecol[(int64_t)el * nrow + t];
            if(col >= 0 && col < ncol)
            {
                oci[ind]  = col;
                oval[ind] = eval[(int64_t)el * nrow + t];
                ++ind;
            }
        }
    }
}
template <typename T, bool SORT>
__global__ __launch_bounds__(kBlock) void k_x2csr_fill_coo(int ngroups, const int* __restrict__ grow,
                                                           const int* __restrict__ gptr,
                                                           const int* __restrict__ ccol,
                                                           const T* __restrict__ cval,
                                                           const int* __restrict__ rp,
                                                           int* __restrict__ oci, T* __restrict__ oval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += gsz)
    {
        const int row = grow[g];
        const int s = gptr[g], e = gptr[g + 1];
        const int base = rp[row + 1] - (e - s); // COO entries close the row
        for(int i = s; i < e; ++i)
        {
            const int col = ccol[i];
            const T   v   = cval[i];
            int       k   = base + (i - s);
            if(SORT) // stable insertion: move strictly greater columns up
                for(; k > base && oci[k - 1] > col; --k)
                {
                    oci[k]  = oci[k - 1];
                    oval[k] = oval[k - 1];
                }
            oci[k]  = col;
            oval[k] = v;
        }
    }
}

static int build_coo_groups(ramd_mat_s* m, const int* rowptr_like)
{
    // rowptr_like: [nrow+1] offsets of every row's COO entries (CSR rp, or the HYB overflow scan)
    Backend& b    = backend();
    int*     flag = nullptr;
    RAMD_TRY(dev_alloc(&flag, (int64_t)m->nrow + 1));
    const int grid = ew_grid((int64_t)m->nrow + 1);
    hipLaunchKernelGGL(k_flag_nonempty, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, rowptr_like, flag);
    int s = device_exclusive_scan(flag, flag, (int64_t)m->nrow + 1);
    int ng = 0;
    if(s == RAMD_OK)
    {
        hipError_t e = hipMemcpyAsync(&ng, flag + m->nrow, sizeof(int), hipMemcpyDeviceToHost, b.cur);
        if(e == hipSuccess)
            e = hipStreamSynchronize(b.cur);
        if(e != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    if(s == RAMD_OK)
        s = dev_alloc(&m->coo_grow, ng);
    if(s == RAMD_OK)
        s = dev_alloc(&m->coo_gptr, (int64_t)ng + 1);
    if(s == RAMD_OK)
    {
        m->coo_ngroups = ng;
        hipLaunchKernelGGL(k_compact_rows, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, rowptr_like,
                           flag, m->coo_grow, m->coo_gptr);
        int        last = (int)m->coo_nnz;
        hipError_t e = hipMemcpyAsync(m->coo_gptr + ng, &last, sizeof(int), hipMemcpyHostToDevice, b.cur);
        if(e == hipSuccess)
            e = hipStreamSynchronize(b.cur);
        if(e != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    dev_free(&flag);
    return s;
}

// (CSR <-> DIA, host_conversion.cpp:958-1113: dia.hip, with the diagonal-wise products.  CSR <-> BCSR: bcsr.hip.  CSR <-> MCSR,
//  host_conversion.cpp:146-323: mcsr.hip, with the diagonal-first products.  DENSE is "not provided by this backend")

template <typename T>
static int convert_from_csr(ramd_mat_s* m, int format)
{
    Backend&  b    = backend();
    const int grid = ew_grid(std::max(m->nrow, 1));
    if(format == RAMD_ELL)
    {
        int* rn = nullptr;
        RAMD_TRY(dev_alloc(&rn, m->nrow));
        hipLaunchKernelGGL(k_row_nnz, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->rp, rn, 0, 0);
        int width = 0;
        int s     = device_max_int(rn, m->nrow, &width);
        dev_free(&rn);
        RAMD_TRY(s);
        if(m->nrow == 0)
            width = 0;
        // host_conversion.cpp:648-651: "Limit ELL size to 5 times CSR nnz" -- integer division
        if(m->nrow > 0 && width > 5 * (m->nnz / m->nrow))
            RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_ell refused: max row nnz > 5 * (nnz / nrow); matrix stays CSR");
        const int64_t nnz_ell = (int64_t)width * m->nrow;
        RAMD_TRY(dev_alloc(&m->ell_col, nnz_ell));
        void* ev = nullptr;
        RAMD_HIP(cached_malloc(&ev, (size_t)nnz_ell * sizeof(T) + kPad));
        m->ell_val   = ev;
        m->ell_width = width;
        if(nnz_ell > 0)
            hipLaunchKernelGGL((k_csr2ell<T>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, width, m->rp,
                               m->ci, (const T*)m->val, m->ell_col, (T*)m->ell_val);
        RAMD_HIP(hipGetLastError());
        RAMD_HIP(hipStreamSynchronize(b.cur));
        mat_free_csr(m);
        m->format = RAMD_ELL;
        m->nnz    = nnz_ell;
        return RAMD_OK;
    }
    if(format == RAMD_HYB)
    {
        if(m->nrow == 0 || m->nnz <= 0)
            RAMD_FAIL(RAMD_ERR_REFUSED, "csr_to_hyb refused: empty matrix (nnz_hyb <= 0)");
        const int     width   = (int)((m->nnz - 1) / m->nrow + 1); // host_conversion.cpp:1131-1135
        const int64_t nnz_ell = (int64_t)width * m->nrow;
        int*          crp     = nullptr;
        RAMD_TRY(dev_alloc(&crp, (int64_t)m->nrow + 1));
        hipLaunchKernelGGL(k_row_nnz, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->rp, crp, width, 1);
        int s    = device_exclusive_scan(crp, crp, (int64_t)m->nrow + 1);
        int ncoo = 0;
        if(s == RAMD_OK)
        {
            hipError_t e = hipMemcpyAsync(&ncoo, crp + m->nrow, sizeof(int), hipMemcpyDeviceToHost, b.cur);
            if(e == hipSuccess)
                e = hipStreamSynchronize(b.cur);
            if(e != hipSuccess)
                s = RAMD_ERR_HIP;
        }
        if(s == RAMD_OK)
            s = dev_alloc(&m->ell_col, nnz_ell);
        void *ev = nullptr, *cv = nullptr;
        if(s == RAMD_OK && cached_malloc(&ev, (size_t)nnz_ell * sizeof(T) + kPad) != hipSuccess)
            s = RAMD_ERR_HIP;
        if(s == RAMD_OK)
            s = dev_alloc(&m->coo_row, ncoo);
        if(s == RAMD_OK)
            s = dev_alloc(&m->coo_col, ncoo);
        if(s == RAMD_OK && cached_malloc(&cv, (size_t)ncoo * sizeof(T) + kPad) != hipSuccess)
            s = RAMD_ERR_HIP;
        if(s != RAMD_OK)
        {
            dev_free(&crp);
            if(ev)
                (void)cached_free(ev);
            if(cv)
                (void)cached_free(cv);
            mat_free_ell(m);
            mat_free_coo(m);
            RAMD_FAIL(s, "csr_to_hyb: allocation failed");
        }
        m->ell_val   = ev;
        m->coo_val   = cv;
        m->ell_width = width;
        m->coo_nnz   = ncoo;
        hipLaunchKernelGGL((k_csr2hyb<T>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, width, m->rp,
                           m->ci, (const T*)m->val, crp, m->ell_col, (T*)m->ell_val, m->coo_row,
                           m->coo_col, (T*)m->coo_val);
        if(ncoo > 0)
            s = build_coo_groups(m, crp);
        hipError_t e = hipStreamSynchronize(b.cur);
        dev_free(&crp);
        RAMD_TRY(s);
        RAMD_HIP(e);
        mat_free_csr(m);
        m->format = RAMD_HYB;
        m->nnz    = nnz_ell + ncoo;
        return RAMD_OK;
    }
    if(format == RAMD_COO)
    {
        RAMD_TRY(dev_alloc(&m->coo_row, m->nnz));
        m->coo_nnz = m->nnz;
        if(m->nnz > 0)
        {
            hipLaunchKernelGGL(k_expand_rows, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->rp,
                               m->coo_row);
            RAMD_TRY(build_coo_groups(m, m->rp));
        }
        RAMD_HIP(hipStreamSynchronize(b.cur));
        // column and value arrays are adopted unchanged (host_conversion.cpp:611-612 copies them)
        m->coo_col = m->ci;
        m->coo_val = m->val;
        m->ci      = nullptr;
        m->val     = nullptr;
        dev_free(&m->rp);
        m->format = RAMD_COO;
        return RAMD_OK;
    }
    RAMD_FAIL(RAMD_ERR_UNSUPPORTED, "conversion target not provided by this backend");
}

template <typename T>
static int convert_to_csr(ramd_mat_s* m)
{
    Backend&  b    = backend();
    const int nrow = m->nrow;
    int*      rp   = nullptr;
    RAMD_TRY(dev_alloc(&rp, (int64_t)nrow + 1));
    const int  grid    = ew_grid((int64_t)nrow + 1);
    const bool has_ell = (m->format == RAMD_ELL || m->format == RAMD_HYB);
    const bool has_coo = (m->format == RAMD_COO || m->format == RAMD_HYB) && m->coo_ngroups > 0;
    hipLaunchKernelGGL(k_x2csr_count_ell, dim3(grid), dim3(kBlock), 0, b.cur, nrow, m->ncol,
                       has_ell ? m->ell_width : 0, m->ell_col, rp);
    if(has_coo)
        hipLaunchKernelGGL(k_x2csr_count_coo, dim3(ew_grid(m->coo_ngroups)), dim3(kBlock), 0, b.cur,
                           m->coo_ngroups, m->coo_grow, m->coo_gptr, rp);
    int s   = device_exclusive_scan(rp, rp, (int64_t)nrow + 1);
    int nnz = 0;
    if(s == RAMD_OK)
    {
        hipError_t e = hipMemcpyAsync(&nnz, rp + nrow, sizeof(int), hipMemcpyDeviceToHost, b.cur);
        if(e == hipSuccess)
            e = hipStreamSynchronize(b.cur);
        if(e != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    int*  ci  = nullptr;
    void* val = nullptr;
    if(s == RAMD_OK)
        s = dev_alloc(&ci, nnz);
    if(s == RAMD_OK && cached_malloc(&val, (size_t)nnz * sizeof(T) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s != RAMD_OK)
    {
        dev_free(&rp);
        dev_free(&ci);
        return s;
    }
    if(has_ell && m->ell_width > 0 && nrow > 0)
        hipLaunchKernelGGL((k_x2csr_fill_ell<T>), dim3(grid), dim3(kBlock), 0, b.cur, nrow, m->ncol, m->ell_width,
                           m->ell_col, (const T*)m->ell_val, rp, ci, (T*)val);
    if(has_coo)
    {
        const int g2 = ew_grid(m->coo_ngroups);
        if(m->format == RAMD_COO)
            hipLaunchKernelGGL((k_x2csr_fill_coo<T, true>), dim3(g2), dim3(kBlock), 0, b.cur, m->coo_ngroups,
                               m->coo_grow, m->coo_gptr, m->coo_col, (const T*)m->coo_val, rp, ci, (T*)val);
        else
            hipLaunchKernelGGL((k_x2csr_fill_coo<T, false>), dim3(g2), dim3(kBlock), 0, b.cur, m->coo_ngroups,
                               m->coo_grow, m->coo_gptr, m->coo_col, (const T*)m->coo_val, rp, ci, (T*)val);
    }
    hipError_t e = hipGetLastError();
    if(e == hipSuccess)
        e = hipStreamSynchronize(b.cur);
    mat_free_ell(m);
    mat_free_coo(m);
    m->rp     = rp;
    m->ci     = ci;
    m->val    = val;
    m->nnz    = nnz;
    m->format = RAMD_CSR;
    RAMD_HIP(e);
    return RAMD_OK;
}

} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_mat_convert(ramd_mat_t m, int format)
{
    RAMD_NARROW_ONLY(m);
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(m->format == format)
        return RAMD_OK;
    if(format == RAMD_BCSR)
        RAMD_FAIL(RAMD_ERR_ARG, "ConvertTo(BCSR) needs a block dimension: ramd_mat_convert_bcsr");
    mat_values_changed(m); // (val moves or is rebuilt)
    if(m->format != RAMD_CSR)
    {
        if(format != RAMD_CSR)
            return RAMD_ERR_UNSUPPORTED; // X -> CSR -> Y goes through the caller (local_matrix.cpp:2085-2093)
        if(m->format == RAMD_BCSR)
            return bcsr_to_csr(m);
        if(m->format == RAMD_DIA)
            return dia_to_csr(m);
        if(m->format == RAMD_MCSR)
            return mcsr_to_csr(m);
        if(m->format != RAMD_ELL && m->format != RAMD_HYB && m->format != RAMD_COO)
            return RAMD_ERR_UNSUPPORTED;
        mat_format_changed(m); // (an ELL dictionary is not a CSR dictionary)
        return (m->dtype == RAMD_F64) ? convert_to_csr<double>(m) : convert_to_csr<float>(m);
    }
    if(format == RAMD_DIA)
        return csr_to_dia(m);
    if(format == RAMD_MCSR)
        return csr_to_mcsr(m);
    if(m->band_dist < 0) // the ELL/HYB kernels walk the rows in the same band-aware order as CSR
        RAMD_TRY(csr_analyse_band(m));
    const int s = (m->dtype == RAMD_F64) ? convert_from_csr<double>(m, format) : convert_from_csr<float>(m, format);
    if(m->format != RAMD_CSR) // (a refused conversion leaves the CSR matrix and what is known about it as they were)
        mat_format_changed(m); // the triangular analyses, and the row patterns and everything derived from them: CSR's
    return s;
}

int ramd_mat_ell_info(ramd_mat_t m, int* width, int64_t* coo_nnz)
{
    if(!m)
        RAMD_FAIL(RAMD_ERR_ARG, "null matrix handle");
    if(width)
        *width = m->ell_width;
    if(coo_nnz)
        *coo_nnz = m->coo_nnz;
    return RAMD_OK;
}

int ramd_mat_copy_ell_to_host(ramd_mat_t m, int32_t* ell_col, void* ell_val)
{
    if(!m || (m->format != RAMD_ELL && m->format != RAMD_HYB))
        RAMD_FAIL(RAMD_ERR_STATE, "matrix has no ELL part");
    Backend&     b = backend();
    const size_t n = (size_t)m->ell_width * m->nrow;
    if(n > 0)
    {
        RAMD_HIP(hipMemcpyAsync(ell_col, m->ell_col, sizeof(int) * n, hipMemcpyDeviceToHost, b.cur));
        RAMD_HIP(hipMemcpyAsync(ell_val, m->ell_val, val_size(m->dtype) * n, hipMemcpyDeviceToHost,
                                b.cur));
        RAMD_HIP(hipStreamSynchronize(b.cur));
    }
    return RAMD_OK;
}

int ramd_mat_copy_coo_to_host(ramd_mat_t m, int32_t* row, int32_t* col, void* val)
{
    if(!m || (m->format != RAMD_COO && m->format != RAMD_HYB))
        RAMD_FAIL(RAMD_ERR_STATE, "matrix has no COO part");
    Backend&     b = backend();
    const size_t n = (size_t)m->coo_nnz;
    if(n > 0)
    {
        RAMD_HIP(hipMemcpyAsync(row, m->coo_row, sizeof(int) * n, hipMemcpyDeviceToHost, b.cur));
        RAMD_HIP(hipMemcpyAsync(col, m->coo_col, sizeof(int) * n, hipMemcpyDeviceToHost, b.cur));
        RAMD_HIP(hipMemcpyAsync(val, m->coo_val, val_size(m->dtype) * n, hipMemcpyDeviceToHost, b.cur));
        RAMD_HIP(hipStreamSynchronize(b.cur));
    }
    return RAMD_OK;
}

int ramd_mat_cast(ramd_mat_t src, ramd_mat_t* out)
{
    if(!src || !out)
        RAMD_FAIL(RAMD_ERR_ARG, "null handle");
    if(src->format != RAMD_CSR && src->format != RAMD_BCSR)
        RAMD_FAIL(RAMD_ERR_STATE, "cast: source must be CSR or BCSR (mixed_precision.cpp:201 uses CopyToCSR); ELL / HYB / COO / DIA / MCSR go "
                                  "through ConvertTo(CSR)");
    const int  dt = (src->dtype == RAMD_F64) ? RAMD_F32 : RAMD_F64;
    ramd_mat_t m  = nullptr;
    RAMD_TRY(ramd_mat_create(dt, &m));
    if(src->format == RAMD_BCSR) // the same block structure, every value cast
    {
        Backend&      b  = backend();
        const int64_t nv = src->nnz;
        void*         v  = nullptr;
        int           s  = dev_alloc(&m->bcsr_rp, (int64_t)src->bcsr_nrowb + 1);
        if(s == RAMD_OK)
            s = dev_alloc(&m->bcsr_ci, src->bcsr_nnzb);
        if(s == RAMD_OK && cached_malloc(&v, (size_t)nv * val_size(dt) + kPad) != hipSuccess)
            s = RAMD_ERR_HIP;
        m->bcsr_val = v;
        if(s == RAMD_OK
           && (hipMemcpyAsync(m->bcsr_rp, src->bcsr_rp, sizeof(int) * ((size_t)src->bcsr_nrowb + 1), hipMemcpyDeviceToDevice, b.cur)
                   != hipSuccess
               || (src->bcsr_nnzb > 0
                   && hipMemcpyAsync(m->bcsr_ci, src->bcsr_ci, sizeof(int) * (size_t)src->bcsr_nnzb, hipMemcpyDeviceToDevice, b.cur)
                          != hipSuccess)))
            s = RAMD_ERR_HIP;
        if(s == RAMD_OK && nv > 0)
        {
            if(dt == RAMD_F32)
                hipLaunchKernelGGL((k_cast_vals<float, double>), dim3(ew_grid(nv)), dim3(kBlock), 0, b.cur, nv, (float*)m->bcsr_val,
                                   (const double*)src->bcsr_val);
            else
                hipLaunchKernelGGL((k_cast_vals<double, float>), dim3(ew_grid(nv)), dim3(kBlock), 0, b.cur, nv, (double*)m->bcsr_val,
                                   (const float*)src->bcsr_val);
            if(hipGetLastError() != hipSuccess)
                s = RAMD_ERR_HIP;
        }
        if(s != RAMD_OK)
        {
            ramd_mat_destroy(m);
            RAMD_FAIL(s, "cast: allocation / copy failed");
        }
        m->format     = RAMD_BCSR;
        m->nrow       = src->nrow;
        m->ncol       = src->ncol;
        m->nnz        = src->nnz;
        m->bcsr_dim   = src->bcsr_dim;
        m->bcsr_nrowb = src->bcsr_nrowb;
        m->bcsr_ncolb = src->bcsr_ncolb;
        m->bcsr_nnzb  = src->bcsr_nnzb;
        *out          = m;
        return RAMD_OK;
    }
    const bool wide = mat_is_wide(src);
    int        s    = wide ? mat_alloc_csr_wide(m, src->nrow, src->ncol, src->nnz) : mat_alloc_csr(m, src->nrow, src->ncol, src->nnz);
    if(s != RAMD_OK)
    {
        ramd_mat_destroy(m);
        return s;
    }
    Backend& b = backend();
    if(wide)
    {
        RAMD_HIP(hipMemcpyAsync(m->rp64, src->rp64, sizeof(int64_t) * ((size_t)src->nrow + 1), hipMemcpyDeviceToDevice, b.cur));
        RAMD_TRY(mat_wide_finish(m));
    }
    else
        RAMD_HIP(hipMemcpyAsync(m->rp, src->rp, sizeof(int) * ((size_t)src->nrow + 1),
                                hipMemcpyDeviceToDevice, b.cur));
    if(src->nnz > 0)
    {
        RAMD_HIP(hipMemcpyAsync(m->ci, src->ci, sizeof(int) * (size_t)src->nnz, hipMemcpyDeviceToDevice,
                                b.cur));
        const int grid = ew_grid(src->nnz);
        if(dt == RAMD_F32)
            hipLaunchKernelGGL((k_cast_vals<float, double>), dim3(grid), dim3(kBlock), 0, b.cur, src->nnz,
                               (float*)m->val, (const double*)src->val);
        else
            hipLaunchKernelGGL((k_cast_vals<double, float>), dim3(grid), dim3(kBlock), 0, b.cur, src->nnz,
                               (double*)m->val, (const float*)src->val);
        RAMD_HIP(hipGetLastError());
    }
    m->pat_off = src->pat_off; // (ramd_mat_pattern_use(src, 0) holds for the value-cast copy too: MixedPrecisionDC's inner operator)
    *out = m;
    return RAMD_OK;
}

int ramd_mat_extract_submatrix(ramd_mat_t m, int r0, int c0, int rs, int cs, ramd_mat_t out)
{
    if(!m || !out || m == out)
        RAMD_FAIL(RAMD_ERR_ARG, "bad handles");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(out->dtype != m->dtype || r0 < 0 || c0 < 0 || rs < 0 || cs < 0 || r0 + rs > m->nrow
       || c0 + cs > m->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "ExtractSubMatrix: range out of bounds / dtype mismatch");
    const SubRule rule{r0, c0, cs};
    const char *  op = "ExtractSubMatrix", *res = "the result";
    return mat_is_wide(m) ? csr_filter(op, res, rule, m, m->rp64, rs, cs, out) : csr_filter(op, res, rule, m, m->rp, rs, cs, out);
}

int ramd_mat_permute(ramd_mat_t m, ramd_vec_t perm)
{
    RAMD_NARROW_ONLY(m);
    if(!m || !perm)
        RAMD_FAIL(RAMD_ERR_ARG, "bad handles");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(perm->dtype != RAMD_I32 || perm->n != m->nrow || m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "Permute: need a square matrix and an int32 permutation of its size");
    if(m->nnz <= 0)
        return RAMD_OK;
    Backend& b   = backend();
    int*     orp = nullptr;
    int*     oci = nullptr;
    void*    ova = nullptr;
    RAMD_TRY(dev_alloc(&orp, (int64_t)m->nrow + 1));
    int s = dev_alloc(&oci, m->nnz);
    if(s == RAMD_OK && cached_malloc(&ova, (size_t)m->nnz * val_size(m->dtype) + kPad) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK)
    {
        const int grid = ew_grid((int64_t)m->nrow + 1);
        hipLaunchKernelGGL(k_perm_row_nnz, dim3(grid), dim3(kBlock), 0, b.cur, m->nrow, m->rp,
                           (const int*)perm->d, orp);
        s = device_exclusive_scan(orp, orp, (int64_t)m->nrow + 1);
        if(s == RAMD_OK)
        {
            if(m->dtype == RAMD_F64)
                hipLaunchKernelGGL((k_perm_fill<double>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow,
                                   m->rp, m->ci, (const double*)m->val, (const int*)perm->d, orp, oci,
                                   (double*)ova);
            else
                hipLaunchKernelGGL((k_perm_fill<float>), dim3(grid), dim3(kBlock), 0, b.cur, m->nrow,
                                   m->rp, m->ci, (const float*)m->val, (const int*)perm->d, orp, oci,
                                   (float*)ova);
            if(hipStreamSynchronize(b.cur) != hipSuccess)
                s = RAMD_ERR_HIP;
        }
    }
    if(s != RAMD_OK)
    {
        dev_free(&orp);
        dev_free(&oci);
        if(ova)
            (void)cached_free(ova);
        RAMD_FAIL(s, "Permute failed");
    }
    mat_free_csr(m);
    mat_free_analysis(m);
    m->rp  = orp;
    m->ci  = oci;
    m->val = ova;
    return RAMD_OK;
}

} // extern "C"
