// csr_filter.hpp -- "a CSR matrix from the entries of another that pass a test": count per output row, exclusive scan, fill.
// One definition for ExtractL/U (matrix_ops.hip), ExtractSubMatrix (convert.hip), Compress (multielim.hip), the direct sum of
// the AS blocks (schwarz.hip) and the strictly lower block part of the BlockPreconditioner (blockprec.hip, offsets only).
//
// A caller states its test as a RULE, a trivially copyable struct that travels to the kernels by value:
//     kRowsOnce                             (static constexpr bool) no source row is read by two output rows
//     Row  row(int64_t i)                   what output row i needs: Row::src, the source row it reads, and whatever keep() and
//                                           col() look at -- computed once per row, not once per entry
//     bool keep(const Row&, int col, T val) does the entry stay?  (a rule that ignores val causes no load of it)
//     int  col(const Row&, int col)         the column a kept entry is written with
// Kept entries keep their storage order.  The result has 32-bit row offsets whatever the source has (P).
#pragma once

#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <climits>
#include <string>
#include <type_traits>
#include <utility>

namespace ramd
{

struct FilterRow // the Row of a rule that needs the source row alone
{
    int src;
};

// lane = output row; cnt[nout] = 0 closes the scan
template <typename P, typename T, typename Rule>
__global__ __launch_bounds__(kBlock) void k_filter_count(int nout, Rule rule, const P* __restrict__ rp, const int* __restrict__ ci,
                                                         const T* __restrict__ val, int* __restrict__ cnt)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nout; i += gsz)
    {
        int c = 0;
        if(i < nout)
        {
            const auto row = rule.row(i);
            for(P j = rp[row.src]; j < rp[row.src + 1]; ++j)
                c += rule.keep(row, ci[j], val[j]) ? 1 : 0;
        }
        cnt[i] = c;
    }
}
template <typename P, typename T, typename Rule>
__global__ __launch_bounds__(kBlock) void k_filter_fill(int nout, Rule rule, const P* __restrict__ rp, const int* __restrict__ ci,
                                                        const T* __restrict__ val, const int* __restrict__ orp, int* __restrict__ oci,
                                                        T* __restrict__ oval)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nout; i += gsz)
    {
        const auto row = rule.row(i);
        int        q   = orp[i];
        for(P j = rp[row.src]; j < rp[row.src + 1]; ++j)
            if(rule.keep(row, ci[j], val[j]))
            {
                oci[q]  = rule.col(row, ci[j]);
                oval[q] = val[j];
                ++q;
            }
    }
}

// Count and scan, then `out` allocated as nrow_out x ncol_out with its row offsets in place or queued on the current stream;
// *nnz = its entries.  One blocking synchronise (the total's way to the host).
//   narrow source (P = int) and Rule::kRowsOnce: the kept entries are at most the source's, so the total fits 32 bits.  The
//     counts are scanned in 32 bits in place and that block BECOMES out->rp; the block allocated for it is the scratch.
//   otherwise: a 64-bit scan, a total beyond INT32_MAX refused (op + ": " + result + " is not provided ..."), the offsets
//     narrowed into out->rp.  Offsets and counts share one scratch block.
// *scratch is the caller's to free (dev_free) AFTER it has synchronised the stream behind its own work: a free waits for the
// device, and in here that would be one more wait between the offsets and the fill.  Set on every path, failures included.
template <typename P, typename T, typename Rule>
int csr_filter_offsets(const char* op, const char* result, const Rule& rule, const P* rp, const int* ci, const T* val, int nrow_out,
                       int ncol_out, ramd_mat_s* out, int64_t* nnz, int** scratch)
{
    constexpr bool narrow = std::is_same<P, int>::value && Rule::kRowsOnce;
    Backend&       b      = backend();
    const int64_t  n1     = (int64_t)nrow_out + 1;
    *nnz                  = 0;
    RAMD_TRY(dev_alloc(scratch, narrow ? n1 : 3 * n1)); // narrow: n1 counts; else n1 64-bit offsets, then the n1 counts
    int64_t* o64 = reinterpret_cast<int64_t*>(*scratch);
    int*     cnt = narrow ? *scratch : *scratch + 2 * n1;
    int      n32 = 0;
    hipLaunchKernelGGL((k_filter_count<P, T, Rule>), dim3(ew_grid(n1)), dim3(kBlock), 0, b.cur, nrow_out, rule, rp, ci, val, cnt);
    int s = hipGetLastError() != hipSuccess ? RAMD_ERR_HIP
            : narrow                        ? device_exclusive_scan(cnt, cnt, n1)
                                            : device_exclusive_scan64(cnt, o64, n1);
    if(s == RAMD_OK
       && ((narrow ? hipMemcpyAsync(&n32, cnt + nrow_out, sizeof(int), hipMemcpyDeviceToHost, b.cur)
                   : hipMemcpyAsync(nnz, o64 + nrow_out, sizeof(int64_t), hipMemcpyDeviceToHost, b.cur))
               != hipSuccess
           || hipStreamSynchronize(b.cur) != hipSuccess))
        s = RAMD_ERR_HIP;
    if(narrow)
        *nnz = n32;
    if(s == RAMD_ERR_HIP)
        set_error(__FILE__, __LINE__, std::string(op) + ": counting the kept entries failed");
    if(s == RAMD_OK && *nnz > INT32_MAX)
    {
        set_error(__FILE__, __LINE__,
                  std::string(op) + ": " + result + " is not provided for 64-bit row offsets (more than INT32_MAX entries)");
        s = RAMD_ERR_UNSUPPORTED;
    }
    if(s == RAMD_OK)
        s = mat_alloc_csr(out, nrow_out, ncol_out, *nnz);
    if(s == RAMD_OK && narrow)
        std::swap(out->rp, *scratch); // (both hold n1 ints; the one that comes back has not been written)
    else if(s == RAMD_OK)
        s = mat_narrow_offsets(o64, out->rp, n1);
    return s;
}

// the fill for one value type, and the synchronise behind it
template <typename T, typename P, typename Rule>
int csr_filter_t(const char* op, const char* result, const Rule& rule, const ramd_mat_s* src, const P* rp, int nrow_out, int ncol_out,
                 ramd_mat_s* out)
{
    Backend& b       = backend();
    const T* val     = (const T*)src->val;
    int64_t  nnz     = 0;
    int*     scratch = nullptr;
    int      s       = csr_filter_offsets(op, result, rule, rp, src->ci, val, nrow_out, ncol_out, out, &nnz, &scratch);
    if(s == RAMD_OK && nnz > 0)
        hipLaunchKernelGGL((k_filter_fill<P, T, Rule>), dim3(ew_grid(nrow_out)), dim3(kBlock), 0, b.cur, nrow_out, rule, rp, src->ci, val,
                           (const int*)out->rp, out->ci, (T*)out->val);
    if(s == RAMD_OK && (hipGetLastError() != hipSuccess || hipStreamSynchronize(b.cur) != hipSuccess))
    {
        set_error(__FILE__, __LINE__, std::string(op) + ": copying the kept entries failed");
        s = RAMD_ERR_HIP;
    }
    dev_free(&scratch);
    return s;
}

// out = the entries of the rows of `src` (row offsets rp: src->rp, or src->rp64 of a wide source) that pass the rule; out has
// src's dtype.  Two blocking synchronises: the one of csr_filter_offsets and one behind the fill; the scratch is freed last
template <typename P, typename Rule>
int csr_filter(const char* op, const char* result, const Rule& rule, const ramd_mat_s* src, const P* rp, int nrow_out, int ncol_out,
               ramd_mat_s* out)
{
    return src->dtype == RAMD_F64 ? csr_filter_t<double>(op, result, rule, src, rp, nrow_out, ncol_out, out)
                                  : csr_filter_t<float>(op, result, rule, src, rp, nrow_out, ncol_out, out);
}

} // namespace ramd
