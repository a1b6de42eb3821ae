// wave_rows.hpp -- the wave-private row walk: a wave stages the entries of ITS 64 rows in an LDS image of its own and walks
// them lane = row.  One definition for k_csr_wr (spmv.hip), k_csr_wide (spmv_wide.hip) and k_tns_tri (tns.hip); a kernel keeps
// its row range, its wave base, its dictionary and its epilogue and calls, per pass of CAP entries,
//     wave_stage_pass  (global -> registers -> the wave's LDS image)        and
//     wave_walk_pass   (LDS image -> gathers -> the row's sum, left to right in storage order).
// No workgroup barrier anywhere: a wave waits for nobody but itself (k_csr_tr's workgroup passes left the waves of a workgroup
// waiting for each other 72 % of their cycles on 27-entry rows, profiles/r06_pmc_csr_tr_lap27.txt), and the x gathers of a step
// stay the 64 consecutive elements of a banded matrix.
//
// Why the code has this shape -- measured on the 27-point operator at 256^3 (tools/spmv_time.py, alternating runs):
//   * wave-private staging instead of workgroup passes: 1.13 -> 1.00 ms;
//   * no load under a branch, in the staging and in the walk: a load under a branch makes the compiler wait for each packet
//     on its own.  Every lane loads every packet (one behind the wave's entries re-reads the pass's first one), and a lane past
//     its row's end reads entry 0 / element 0 and keeps its sum by a select: 0.98 -> 0.90 ms;
//   * the walk in three separate phases per turn -- GW LDS reads, then GW gathers, then GW selects: all gathers of a turn are
//     in flight before the first product.  Fused per entry the gathers would be serialised behind each other's use;
//   * the compact copy of the 64-row offsets, gather widths of 8 / 14 / 28 and half-size passes at twice the occupancy:
//     nothing (+-2 %).
// The same select form inside k_csr_tr (workgroup passes, 7-entry rows at 512^3): 2.38-2.39 -> 2.43-2.51 ms -- this walk is for
// wave-private images only.
// Addressing: val / ci may be larger than 4 GiB (spmv_wide.hip), so nothing here addresses them from the array base.  The
// caller forms ONE base per wave -- its first entry rounded down to a 16-byte packet of both arrays -- and positions, passes
// and row ranges are 32-bit offsets from it.
#pragma once

#include "device_utils.hpp"
#include "matrix_impl.hpp"

namespace ramd
{

// Stages the pass [cb, cb + CAP) of the wave's entries [0, lend): columns from cw into sc (COLS = false: a row-pattern kernel,
// no columns read), values from vw into sv.  All packets are requested before the first is stored.
template <typename T, int CAP, bool COLS>
__device__ __forceinline__ void wave_stage_pass(const int* cw, const T* vw, int cb, int lend, int lane, int* sc, T* sv)
{
    using VP         = typename Pack<T>::type;
    constexpr int VN = Pack<T>::N;
    v4i32         c[CAP / (4 * 64)];
    VP            a[CAP / (VN * 64)];
#pragma unroll
    for(int k = 0; k < (COLS ? CAP / (4 * 64) : 0); ++k)
    {
        const int j = cb + (k * 64 + lane) * 4;
        c[k]        = nt_load(reinterpret_cast<const v4i32*>(cw + (j < lend ? j : cb)));
    }
#pragma unroll
    for(int k = 0; k < CAP / (VN * 64); ++k)
    {
        const int j = cb + (k * 64 + lane) * VN;
        a[k]        = nt_load(reinterpret_cast<const VP*>(vw + (j < lend ? j : cb)));
    }
#pragma unroll
    for(int k = 0; k < (COLS ? CAP / (4 * 64) : 0); ++k)
    {
        const int g = (k * 64 + lane) * 4;
        if(cb + g < lend)
            *reinterpret_cast<v4i32*>(sc + g) = c[k];
    }
#pragma unroll
    for(int k = 0; k < CAP / (VN * 64); ++k)
    {
        const int g = (k * 64 + lane) * VN;
        if(cb + g < lend)
            *reinterpret_cast<VP*>(sv + g) = a[k];
    }
    __builtin_amdgcn_wave_barrier();
}

// Walks the lane's `len` entries of the staged pass, the first at position `first` of the image (len <= 0: nothing of the row
// in this pass), GW at a time, and returns the row's sum.
//   col_of(idx, k, ok)  column of the entry at image position idx, the k-th of the row in this pass; idx = 0 where !ok, and a
//                       dictionary then reads its element 0 too.  May clear ok (k_tns_tri<UPPER>: col > row); the column of
//                       an entry that is not ok is not used.
//   gather(col)         what the term needs from memory: x[col], or a pair of elements
//   term(sum, v, g)     the sum with the entry's product added; kept only where ok
template <typename T, int GW, typename ColOf, typename Gather, typename Term>
__device__ __forceinline__ T wave_walk_pass(const T* sv, int first, int len, T sum, ColOf col_of, Gather gather, Term term)
{
    for(int jb = 0; __ballot(jb < len) != 0ull; jb += GW)
    {
        int  cc[GW];
        T    v[GW];
        bool ok[GW];
        decltype(gather(0)) g[GW];
#pragma unroll
        for(int e = 0; e < GW; ++e)
        {
            ok[e]         = jb + e < len;
            const int idx = ok[e] ? first + jb + e : 0;
            v[e]          = sv[idx];
            const int col = col_of(idx, jb + e, ok[e]);
            cc[e]         = ok[e] ? col : 0;
        }
#pragma unroll
        for(int e = 0; e < GW; ++e)
            g[e] = gather(cc[e]);
#pragma unroll
        for(int e = 0; e < GW; ++e)
        {
            const T s2 = term(sum, v[e], g[e]);
            sum        = ok[e] ? s2 : sum;
        }
    }
    __builtin_amdgcn_wave_barrier(); // (the next pass overwrites the image)
    return sum;
}

// The walk of the CSR products (k_csr_wr, k_csr_wide) over the row's entries [lo, hi) of the pass at cb: the column is the
// stored one (sc) or, PAT, row + the dictionary's offset (scol; dbase = where the row's offsets start in it, minus the row's
// first position); MODE 1 (y += scalar * A x) scales term by term as the host ApplyAdd does.
template <typename T, int MODE, bool PAT, int GW>
__device__ __forceinline__ T csr_walk_pass(const T* sv, const int* sc, const int* scol, int row, int dbase, int lo, int hi, int cb,
                                           const T* x, T scalar, T sum)
{
    return wave_walk_pass<T, GW>(
        sv, lo - cb, hi - lo, sum,
        [&](int idx, int k, bool& ok) { return PAT ? row + scol[ok ? dbase + lo + k : 0] : sc[idx]; },
        [&](int col) { return x[col]; },
        [&](T s, T v, T xv) { return MODE != 1 ? s + v * xv : s + scalar * v * xv; });
}

// The row epilogue of the CSR products: MODE 2 turns the sum into a damped-Jacobi sweep y = x + scalar * (dinv * (-(A x) +
// rhs)); y is stored non-temporal, unconditionally (a run-time switch let the compiler merge both forms into ONE plain store);
// DOT: one partial of <dotv or x, y> per WAVE, fire-and-forget -- reduce_sum_to_slot adds them in their fixed order.  xrow is
// x[row] where the dot runs against x or MODE is 2.  Called by whole waves (live: the lane has a row).
template <typename T, int MODE, bool DOT>
__device__ __forceinline__ void csr_row_epilogue(bool live, int blk, int row, T sum, T xrow, T* y, T scalar, const CsrDotWs& ws)
{
    double dacc = 0.0;
    if(live)
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
    if(DOT)
    {
        const double wsum = wave_reduce_sum(dacc);
        if((threadIdx.x & 63) == 0)
            ws.part1[blk * (kBlock / 64) + (threadIdx.x >> 6)] = wsum;
    }
}

} // namespace ramd
