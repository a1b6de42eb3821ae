// spmv_lattice.hip -- the value-pattern CSR product of a 5- / 7-point lattice operator: tiles of x in LDS, marched along z.
//
// k_csr_patv (spmv.hip) treats such an operator as a bag of rows: seven 8-byte gathers per row, five of them on lines no
// neighbouring lane has brought in.  Here a workgroup owns an (x, y) tile and a run of z planes (k_mc_rb's geometry, mcsgs.hip):
// it reads every element of x once -- plus a one-cell ring per plane and two planes per run -- by loads of whole lines, takes
// x +- 1 and x +- nx from the plane in LDS and x +- nx ny from registers.
//
// Cells are addressed LINEARLY: the cell left of row r holds x[r - 1], the one above x[r - nx], the plane before x[r - nx ny],
// whether or not that position exists on the lattice (loaded where 0 <= index < n, +0 elsewhere).  A dictionary offset is a
// linear offset and a valid matrix has no column outside [0, n), so the product is right for EVERY matrix whose dictionary
// passed csr_analyse_lattice, wherever its boundary rows lie: nothing about a row's position is verified or assumed.  A slot a
// row's pattern does not have contributes no term (masked, not multiplied by zero).
//
// Bits: the row sum starts from (T)0 and adds v * x slot by slot in ascending column order, every operation rounded once
// (-ffp-contract=off) -- k_csr_patv's sum of a row stored in ascending columns (csr_analyse_lattice admits no other).  The
// fused dot: nx is a multiple of 64, so the 64 lanes of a wave are the rows 64 w .. 64 w + 63 in lane order, and their partial
// goes to ws.part1[w] as k_csr_patv's does.
#include "device_utils.hpp"
#include "spmv_lattice.hpp"

#include <algorithm>

namespace ramd
{

// Two cells per thread: with four (128 x 16 on 512 threads) the kernel with the fused dot needs 136 VGPRs, one workgroup per CU,
// and takes 0.98 ms at 512^3; with two, 78 VGPRs and 0.53 ms.  Only this instantiation is built.  Tiles (128 x 16, 128 x 8,
// 64 x 16) and runs (16 / 32 / 64 planes) measured at 512^3: profiles/lattice_spmv.md
constexpr int kLatTX = 128, kLatTY = 8, kLatThreads = 512, kLatChunkMin = 16, kLatChunkMax = 64;

struct LatDims
{
    int     nx, ny, nz, tiles_x, tiles_y, chunk, npat;
    int64_t n;
};

// waits for LDS only: the loads of the next plane stay in flight across it (k_mc_rb's rb_barrier)
__device__ __forceinline__ void lat_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <typename T, bool DOT, int TX, int TY, int NT>
__global__ __launch_bounds__(NT) void k_csr_lat(LatDims g, const T* __restrict__ x, T* __restrict__ y,
                                                const unsigned char* __restrict__ id, const T* __restrict__ vals, CsrDotWs ws)
{
    static_assert(TX % 64 == 0 && NT % 64 == 0 && ((TX / 64) * TY) % (NT / 64) == 0, "a wave owns whole 64-row runs");
    constexpr int RX = TX / 64, NW = NT / 64, CPT = RX * TY / NW; // runs per tile line, waves, runs (= cells of a thread) per plane
    constexpr int PX = TX + 2, PC = PX * (TY + 2); // a plane in LDS: the tile and its ring
    constexpr int RING = 2 * TX + 2 * TY, NRG = (RING + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) char lat_lds[];
    T* XP = reinterpret_cast<T*>(lat_lds); // [2][PC]: plane z in XP[z & 1]
    T* SV = XP + 2 * PC; // [npat][kLatSlotW]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup w runs on XCD w % 8: every XCD gets a contiguous run of tiles (the rings of neighbouring tiles meet in one L2)
    int wg = blockIdx.x;
    if(gridDim.x % 8 == 0)
        wg = (wg % 8) * (int)(gridDim.x / 8) + wg / 8;
    const int     tx = wg % g.tiles_x, ty = (wg / g.tiles_x) % g.tiles_y, cz = wg / (g.tiles_x * g.tiles_y);
    const int     x0t = tx * TX, y0t = ty * TY, z0 = cz * g.chunk, z1 = min(z0 + g.chunk, g.nz);
    const int64_t pl = (int64_t)g.nx * g.ny, n = g.n;
    // a thread's cells: lane `lane` of the runs wave, wave + NW, ...  own: a row of this tile; ld: a position an own row reads
    int64_t off[CPT], roff[NRG];
    int     lpos[CPT], rpos[NRG];
    bool    own[CPT], ld[CPT], rld[NRG];
#pragma unroll
    for(int i = 0; i < CPT; ++i)
    {
        const int r = wave + NW * i, lx = (r % RX) * 64 + lane, ly = r / RX, gx = x0t + lx, gy = y0t + ly;
        own[i]  = gx < g.nx && gy < g.ny;
        ld[i]   = gx <= g.nx && gy <= g.ny;
        off[i]  = ld[i] ? (int64_t)gy * g.nx + gx : 0;
        lpos[i] = (ly + 1) * PX + lx + 1;
    }
#pragma unroll
    for(int j = 0; j < NRG; ++j)
    {
        const int q = tid + NT * j;
        int       lx, ly;
        if(q < TX)
            lx = q, ly = -1;
        else if(q < 2 * TX)
            lx = q - TX, ly = TY;
        else if(q < 2 * TX + TY)
            lx = -1, ly = q - 2 * TX;
        else
            lx = TX, ly = q - 2 * TX - TY;
        rld[j]  = q < RING;
        roff[j] = rld[j] ? (int64_t)(y0t + ly) * g.nx + (x0t + lx) : 0;
        rpos[j] = (ly + 1) * PX + lx + 1;
    }
    for(int i = tid; i < g.npat * kLatSlotW; i += NT)
        SV[i] = vals[i];
    const T* dotv = DOT ? static_cast<const T*>(ws.dotv) : nullptr;
#define LAT_X(idx) (((idx) >= 0 && (idx) < n) ? x[(idx)] : (T)0)
    T   xm[CPT], xc[CPT], xp[CPT], xn[CPT], rc[NRG], rn[NRG], dc[CPT], dn[CPT];
    int pc[CPT], pn[CPT];
    {
        const int64_t pb = (int64_t)z0 * pl;
        T             r0[NRG];
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            const int64_t c = pb + off[i];
            xm[i] = ld[i] ? LAT_X(c - pl) : (T)0;
            xc[i] = ld[i] ? LAT_X(c) : (T)0;
            xp[i] = ld[i] ? LAT_X(c + pl) : (T)0;
            pc[i] = own[i] ? (int)id[c] : 0;
            dc[i] = (dotv && own[i]) ? dotv[c] : (T)0;
        }
#pragma unroll
        for(int j = 0; j < NRG; ++j)
        {
            const int64_t c = pb + roff[j];
            r0[j] = rld[j] ? LAT_X(c) : (T)0;
            rc[j] = (rld[j] && z0 + 1 < z1) ? LAT_X(c + pl) : (T)0;
        }
        T* B = XP + (z0 & 1) * PC;
#pragma unroll
        for(int i = 0; i < CPT; ++i)
            if(ld[i])
                B[lpos[i]] = xc[i];
#pragma unroll
        for(int j = 0; j < NRG; ++j)
            if(rld[j])
                B[rpos[j]] = r0[j];
    }
    lat_barrier();
    for(int z = z0; z < z1; ++z)
    {
        const int64_t pb   = (int64_t)z * pl;
        const bool    more = z + 1 < z1;
        // the loads of the planes ahead go out before this plane is computed: x of z + 2 (the registers' z + 1 of the next
        // step), the ring of z + 2, the pattern ids of z + 1
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            const int64_t c = pb + off[i];
            xn[i] = (more && ld[i]) ? LAT_X(c + 2 * pl) : (T)0;
            pn[i] = (more && own[i]) ? (int)id[c + pl] : 0;
            dn[i] = (more && dotv && own[i]) ? dotv[c + pl] : (T)0;
        }
#pragma unroll
        for(int j = 0; j < NRG; ++j)
        {
            const int64_t c = pb + 2 * pl + roff[j];
            rn[j] = (rld[j] && z + 2 < z1) ? LAT_X(c) : (T)0;
        }
        const T* B = XP + (z & 1) * PC;
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            if(!own[i]) // (the whole run: wave-uniform)
                continue;
            const int64_t row = pb + off[i];
            const T*      tv  = SV + pc[i] * kLatSlotW;
            const T*      C   = B + lpos[i];
            const int     mk  = (int)tv[kLatSlots];
            T             s   = (T)0;
            if(mk & 1)
                s += tv[0] * xm[i];
            if(mk & 2)
                s += tv[1] * C[-PX];
            if(mk & 4)
                s += tv[2] * C[-1];
            if(mk & 8)
                s += tv[3] * xc[i];
            if(mk & 16)
                s += tv[4] * C[1];
            if(mk & 32)
                s += tv[5] * C[PX];
            if(mk & 64)
                s += tv[6] * xp[i];
            nt_store(s, y + row);
            if(DOT)
            {
                const double  wsum = wave_reduce_sum((double)s * (double)(dotv ? dc[i] : xc[i]));
                const int64_t w    = row >> 6; // (lane 0's row is a multiple of 64)
                if(lane == 0)
                    ws.part1[w] = wsum;
                // the last run also clears what is left of its 256-row block's four partials (k_csr_patv: waves without rows)
                else if(row - lane + 64 == n && lane < 4 && ((w + lane) >> 2) == (w >> 2))
                    ws.part1[w + lane] = 0.0;
            }
        }
        if(more)
        {
            T* W = XP + ((z + 1) & 1) * PC;
#pragma unroll
            for(int i = 0; i < CPT; ++i)
                if(ld[i])
                    W[lpos[i]] = xp[i];
#pragma unroll
            for(int j = 0; j < NRG; ++j)
                if(rld[j])
                    W[rpos[j]] = rc[j];
        }
        lat_barrier();
#pragma unroll
        for(int i = 0; i < CPT; ++i)
            xm[i] = xc[i], xc[i] = xp[i], xp[i] = xn[i], pc[i] = pn[i], dc[i] = dn[i];
#pragma unroll
        for(int j = 0; j < NRG; ++j)
            rc[j] = rn[j];
    }
#undef LAT_X
}

// CG + Jacobi on a lattice operator: the direction update of one iteration and the product of the next in one pass over p.
//   pn = beta p + d r ; x += alpha p ; q = A pn ; <pn, q>          (k_cg_direction_dc, fused.hip, then k_csr_lat<DOT>)
// k_csr_lat's geometry, LDS planes, barriers and look-ahead; where that kernel loads x[c] this one loads p[c], r[c] and the
// code of d and forms pn = beta * p[c] + d * r[c] -- k_cg_direction_dc's expression, every operation rounded once -- which
// takes x's place in LDS and in the registers.  Ring cells and seam planes form the same expression from the same operands,
// so they hold the bits their owner stores.  A position outside [0, n) is +0, not computed from anything.
// pn goes to ANOTHER buffer than p: neighbouring workgroups read p at ring and seam positions at times nobody orders.  x is
// read and written by the owner of a cell only (in place); r, the codes and the pattern ids are read only.
// The loads of plane z + 2 stay raw (p, r, code, x) across the product of plane z and are formed after its barrier, so no
// wait for them stands before the product.  The partial of <pn, q> per 64-row run goes to ws.part1 as k_csr_lat<DOT>'s does
// without dotv: same lanes, same tree, same slot.
// XM, what a launch does with x (nothing inside an iteration reads x, and the buffer pn goes to still holds the p of two
// launches ago at a cell until its owner stores there):
//   kCgXEach   x += alpha p                                    (the expressions above)
//   kCgXDefer  x is neither loaded nor stored; alpha goes to *alpha_out (one lane of one workgroup, nothing reads it here)
//   kCgXBoth   x = (x + a_prev pw_old) + alpha p: a_prev the alpha a deferring launch kept in s[slot_alpha], pw_old what the
//              owner of a cell finds in pw before it stores pn there -- loaded with the look-ahead, by the thread that stores.
//              The two steps are the two roundings of two kCgXEach launches.
// pn, q, the partials and every ring and seam cell are the same in all three.
// a + b with a as the FIRST operand of the instruction.  Where both operands are NaNs of different bits the sum takes the
// first one's, and the compiler orders the operands of an addition as it likes -- differently at different places of one
// kernel.  The update of x is written this way so that a cell gets the same bits whichever launch, and whichever place of
// the kernel, adds to it (alpha is itself a NaN once a NaN has reached a reduction, so such pairs do meet).
__device__ __forceinline__ double lat_add_in_order(double a, double b)
{
    double s;
    asm("v_add_f64 %0, %1, %2" : "=v"(s) : "v"(a), "v"(b));
    return s;
}
__device__ __forceinline__ float lat_add_in_order(float a, float b)
{
    float s;
    asm("v_add_f32_e32 %0, %1, %2" : "=v"(s) : "v"(a), "v"(b));
    return s;
}
// ... and a * b likewise
__device__ __forceinline__ double lat_mul_in_order(double a, double b)
{
    double s;
    asm("v_mul_f64 %0, %1, %2" : "=v"(s) : "v"(a), "v"(b));
    return s;
}
__device__ __forceinline__ float lat_mul_in_order(float a, float b)
{
    float s;
    asm("v_mul_f32_e32 %0, %1, %2" : "=v"(s) : "v"(a), "v"(b));
    return s;
}

template <typename T, bool CODED, bool NTS, int XM, int TX, int TY, int NT>
__global__ __launch_bounds__(NT) void k_cg_lat(LatDims g, T* __restrict__ x, const T* __restrict__ po, T* __restrict__ pw,
                                               const T* __restrict__ r, T* __restrict__ y, T duni, const T* __restrict__ table,
                                               int count, const unsigned char* __restrict__ codes,
                                               const double* __restrict__ scalars, int slot_rho, int slot_pq, int slot_new,
                                               const unsigned char* __restrict__ id, const T* __restrict__ vals, CsrDotWs ws,
                                               int slot_alpha, double* alpha_out)
{
    static_assert(XM == kCgXEach || XM == kCgXDefer || XM == kCgXBoth, "the x mode");
    static_assert(TX % 64 == 0 && NT % 64 == 0 && ((TX / 64) * TY) % (NT / 64) == 0, "a wave owns whole 64-row runs");
    constexpr int RX = TX / 64, NW = NT / 64, CPT = RX * TY / NW;
    constexpr int PX = TX + 2, PC = PX * (TY + 2);
    constexpr int RING = 2 * TX + 2 * TY, NRG = (RING + NT - 1) / NT;
    extern __shared__ __attribute__((aligned(16))) char lat_lds[];
    T* XP = reinterpret_cast<T*>(lat_lds); // [2][PC]: pn of plane z in XP[z & 1]
    T* SV = XP + 2 * PC; // [npat][kLatSlotW]
    T* DT = SV + g.npat * kLatSlotW; // [count] the table of d (CODED)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int       wg  = blockIdx.x;
    if(gridDim.x % 8 == 0)
        wg = (wg % 8) * (int)(gridDim.x / 8) + wg / 8;
    const int     tx = wg % g.tiles_x, ty = (wg / g.tiles_x) % g.tiles_y, cz = wg / (g.tiles_x * g.tiles_y);
    const int     x0t = tx * TX, y0t = ty * TY, z0 = cz * g.chunk, z1 = min(z0 + g.chunk, g.nz);
    const int64_t pl = (int64_t)g.nx * g.ny, n = g.n;
    const T       alpha = (T)scalars[slot_rho] / (T)scalars[slot_pq];
    const T       beta  = (T)scalars[slot_new] / (T)scalars[slot_rho];
    const T       aprev = XM == kCgXBoth ? (T)scalars[slot_alpha] : (T)0;
    if(XM == kCgXDefer && blockIdx.x == 0 && tid == 0)
        *alpha_out = (double)alpha;
    int64_t off[CPT], roff[NRG];
    int     lpos[CPT], rpos[NRG];
    bool    own[CPT], ld[CPT], rld[NRG];
#pragma unroll
    for(int i = 0; i < CPT; ++i)
    {
        const int rr = wave + NW * i, lx = (rr % RX) * 64 + lane, ly = rr / RX, gx = x0t + lx, gy = y0t + ly;
        own[i]  = gx < g.nx && gy < g.ny;
        ld[i]   = gx <= g.nx && gy <= g.ny;
        off[i]  = ld[i] ? (int64_t)gy * g.nx + gx : 0;
        lpos[i] = (ly + 1) * PX + lx + 1;
    }
#pragma unroll
    for(int j = 0; j < NRG; ++j)
    {
        const int q = tid + NT * j;
        int       lx, ly;
        if(q < TX)
            lx = q, ly = -1;
        else if(q < 2 * TX)
            lx = q - TX, ly = TY;
        else if(q < 2 * TX + TY)
            lx = -1, ly = q - 2 * TX;
        else
            lx = TX, ly = q - 2 * TX - TY;
        rld[j]  = q < RING;
        roff[j] = rld[j] ? (int64_t)(y0t + ly) * g.nx + (x0t + lx) : 0;
        rpos[j] = (ly + 1) * PX + lx + 1;
    }
    for(int i = tid; i < g.npat * kLatSlotW; i += NT)
        SV[i] = vals[i];
    if(CODED)
        for(int i = tid; i < count; i += NT)
            DT[i] = table[i];
    lat_barrier(); // (DT is read before the first plane is in LDS)
    // a position as loaded (p, r, the code of d) and formed; `in`: the position is loaded at all and lies in [0, n)
#define CGL_LOAD(in, c, P, R, K)                                \
    do                                                          \
    {                                                           \
        const bool in_ = (in) && (c) >= 0 && (c) < n;           \
        P              = in_ ? po[(c)] : (T)0;                  \
        R              = in_ ? r[(c)] : (T)0;                   \
        K              = (CODED && in_) ? (int)codes[(c)] : 0;  \
    } while(0)
#define CGL_FORM(in, c, P, R, K, OUT)                           \
    do                                                          \
    {                                                           \
        const T d_  = CODED ? DT[(K)] : duni;                   \
        const T zn_ = d_ * (R);                                 \
        const T pn_ = beta * (P) + zn_;                         \
        OUT         = ((in) && (c) >= 0 && (c) < n) ? pn_ : (T)0; \
    } while(0)
    // an owned row: the new p stored, x updated with the old one (kCgXBoth: first with PW, what pw held; kCgXDefer: not at all)
#define CGL_OWNED(c, P, PN, X, PW)                              \
    do                                                          \
    {                                                           \
        const T x0_ = XM == kCgXBoth ? lat_add_in_order((X), lat_mul_in_order(aprev, (PW))) : (X); \
        const T xn_ = lat_add_in_order(x0_, lat_mul_in_order(alpha, (P))); \
        if(NTS)                                                 \
        {                                                       \
            nt_store((PN), pw + (c));                           \
            if(XM != kCgXDefer)                                 \
                nt_store(xn_, x + (c));                         \
        }                                                       \
        else                                                    \
        {                                                       \
            pw[(c)] = (PN);                                     \
            if(XM != kCgXDefer)                                 \
                x[(c)] = xn_;                                   \
        }                                                       \
    } while(0)
    T   xm[CPT], xc[CPT], xp[CPT], rc[NRG];
    T   lp[CPT], lr[CPT], lx_[CPT], lw_[CPT], rlp[NRG], rlr[NRG]; // the look-ahead, raw (lw_: pw as found, kCgXBoth)
    int lk[CPT], rlk[NRG], pc[CPT], pn[CPT];
    {
        const int64_t pb = (int64_t)z0 * pl;
        T             r0[NRG];
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            const int64_t c = pb + off[i];
            T             p0, q0, p1, q1, x0 = (T)0, x1 = (T)0, w0 = (T)0, w1 = (T)0;
            int           k0, k1;
            CGL_LOAD(ld[i], c - pl, lp[i], lr[i], lk[i]);
            CGL_LOAD(ld[i], c, p0, q0, k0);
            CGL_LOAD(ld[i], c + pl, p1, q1, k1);
            const bool two = own[i] && z0 + 1 < z1;
            if(XM != kCgXDefer && own[i])
                x0 = nt_load(x + c);
            if(XM != kCgXDefer && two)
                x1 = nt_load(x + c + pl);
            if(XM == kCgXBoth && own[i])
                w0 = nt_load(pw + c);
            if(XM == kCgXBoth && two)
                w1 = nt_load(pw + c + pl);
            pc[i] = own[i] ? (int)id[c] : 0;
            CGL_FORM(ld[i], c - pl, lp[i], lr[i], lk[i], xm[i]);
            CGL_FORM(ld[i], c, p0, q0, k0, xc[i]);
            CGL_FORM(ld[i], c + pl, p1, q1, k1, xp[i]);
            if(own[i])
                CGL_OWNED(c, p0, xc[i], x0, w0);
            if(two)
                CGL_OWNED(c + pl, p1, xp[i], x1, w1);
        }
#pragma unroll
        for(int j = 0; j < NRG; ++j)
        {
            const int64_t c = pb + roff[j];
            CGL_LOAD(rld[j], c, rlp[j], rlr[j], rlk[j]);
            CGL_FORM(rld[j], c, rlp[j], rlr[j], rlk[j], r0[j]);
            const bool nx_ = rld[j] && z0 + 1 < z1;
            CGL_LOAD(nx_, c + pl, rlp[j], rlr[j], rlk[j]);
            CGL_FORM(nx_, c + pl, rlp[j], rlr[j], rlk[j], rc[j]);
        }
        T* B = XP + (z0 & 1) * PC;
#pragma unroll
        for(int i = 0; i < CPT; ++i)
            if(ld[i])
                B[lpos[i]] = xc[i];
#pragma unroll
        for(int j = 0; j < NRG; ++j)
            if(rld[j])
                B[rpos[j]] = r0[j];
    }
    lat_barrier();
    for(int z = z0; z < z1; ++z)
    {
        const int64_t pb   = (int64_t)z * pl;
        const bool    more = z + 1 < z1, more2 = z + 2 < z1;
        // the loads of the planes ahead go out before this plane is computed: p, r and the code of z + 2 (and x where the
        // plane is this run's), the ring of z + 2, the pattern ids of z + 1
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            const int64_t c = pb + off[i];
            CGL_LOAD(more && ld[i], c + 2 * pl, lp[i], lr[i], lk[i]);
            lx_[i] = (XM != kCgXDefer && more2 && own[i]) ? nt_load(x + c + 2 * pl) : (T)0;
            lw_[i] = (XM == kCgXBoth && more2 && own[i]) ? nt_load(pw + c + 2 * pl) : (T)0;
            pn[i]  = (more && own[i]) ? (int)id[c + pl] : 0;
        }
#pragma unroll
        for(int j = 0; j < NRG; ++j)
        {
            const int64_t c = pb + 2 * pl + roff[j];
            CGL_LOAD(rld[j] && more2, c, rlp[j], rlr[j], rlk[j]);
        }
        const T* B = XP + (z & 1) * PC;
        T        s[CPT];
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            s[i] = (T)0;
            if(!own[i]) // (the whole run: wave-uniform)
                continue;
            const T*  tv = SV + pc[i] * kLatSlotW;
            const T*  C  = B + lpos[i];
            const int mk = (int)tv[kLatSlots];
            T         a  = (T)0;
            if(mk & 1)
                a += tv[0] * xm[i];
            if(mk & 2)
                a += tv[1] * C[-PX];
            if(mk & 4)
                a += tv[2] * C[-1];
            if(mk & 8)
                a += tv[3] * xc[i];
            if(mk & 16)
                a += tv[4] * C[1];
            if(mk & 32)
                a += tv[5] * C[PX];
            if(mk & 64)
                a += tv[6] * xp[i];
            s[i] = a;
            nt_store(a, y + pb + off[i]);
        }
        // the partials of a thread's runs after all its row sums: the reduction trees of the runs are independent of each
        // other (k_csr_lat<DOT>'s partial per run, lane for lane)
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            if(!own[i])
                continue;
            const int64_t row  = pb + off[i];
            const double  wsum = wave_reduce_sum((double)s[i] * (double)xc[i]);
            const int64_t w    = row >> 6; // (lane 0's row is a multiple of 64)
            if(lane == 0)
                ws.part1[w] = wsum;
            // the last run also clears what is left of its 256-row block's four partials (k_csr_patv: waves without rows)
            else if(row - lane + 64 == n && lane < 4 && ((w + lane) >> 2) == (w >> 2))
                ws.part1[w + lane] = 0.0;
        }
        if(more)
        {
            T* W = XP + ((z + 1) & 1) * PC;
#pragma unroll
            for(int i = 0; i < CPT; ++i)
                if(ld[i])
                    W[lpos[i]] = xp[i];
#pragma unroll
            for(int j = 0; j < NRG; ++j)
                if(rld[j])
                    W[rpos[j]] = rc[j];
        }
        lat_barrier();
#pragma unroll
        for(int i = 0; i < CPT; ++i)
        {
            const int64_t c = pb + 2 * pl + off[i];
            xm[i] = xc[i], xc[i] = xp[i], pc[i] = pn[i];
            CGL_FORM(more && ld[i], c, lp[i], lr[i], lk[i], xp[i]);
            if(more2 && own[i])
                CGL_OWNED(c, lp[i], xp[i], lx_[i], lw_[i]);
        }
#pragma unroll
        for(int j = 0; j < NRG; ++j)
        {
            const int64_t c = pb + 2 * pl + roff[j];
            CGL_FORM(rld[j] && more2, c, rlp[j], rlr[j], rlk[j], rc[j]);
        }
    }
#undef CGL_LOAD
#undef CGL_FORM
#undef CGL_OWNED
}

// the tiling of a launch: tiles in x and y, runs of planes along z -> workgroups
template <int TX, int TY>
static int lat_geometry(const ramd_mat_s* m, int chunk_min, int chunk_max, LatDims* out)
{
    Backend& b = backend();
    LatDims  g;
    g.nx = m->lat_dims[0], g.ny = m->lat_dims[1], g.nz = m->lat_dims[2], g.npat = m->pat_n, g.n = m->nrow;
    g.tiles_x = (g.nx + TX - 1) / TX, g.tiles_y = (g.ny + TY - 1) / TY;
    // runs of planes: four workgroups per CU where the lattice has them (a run reads two planes of its neighbours again)
    const int tiles = g.tiles_x * g.tiles_y;
    const int want  = (4 * b.num_cu + tiles - 1) / tiles;
    g.chunk         = std::min(chunk_max, std::max(chunk_min, (g.nz + want - 1) / want));
    *out            = g;
    return tiles * ((g.nz + g.chunk - 1) / g.chunk);
}

template <typename T, int TX, int TY, int NT>
static void lat_launch(const ramd_mat_s* m, const T* x, T* y, bool dot, CsrDotWs ws, int chunk_min, int chunk_max)
{
    Backend&     b = backend();
    LatDims      g;
    const int    blocks = lat_geometry<TX, TY>(m, chunk_min, chunk_max, &g);
    const size_t lds    = sizeof(T) * (size_t)(2 * (TX + 2) * (TY + 2) + g.npat * kLatSlotW);
    if(dot)
        hipLaunchKernelGGL((k_csr_lat<T, true, TX, TY, NT>), dim3((unsigned)blocks), dim3(NT), lds, b.cur, g, x, y,
                           m->pat_id, (const T*)m->lat_vals, ws);
    else
        hipLaunchKernelGGL((k_csr_lat<T, false, TX, TY, NT>), dim3((unsigned)blocks), dim3(NT), lds, b.cur, g, x, y,
                           m->pat_id, (const T*)m->lat_vals, ws);
}

template <typename T>
int launch_csr_lat(const ramd_mat_s* m, const T* x, T* y, bool dot, CsrDotWs ws)
{
    if(m->lat_state != 1 || !m->lat_vals || !m->pat_id)
        RAMD_FAIL(RAMD_ERR_ARG, "launch_csr_lat: the matrix is not in lattice state 1");
    lat_launch<T, kLatTX, kLatTY, kLatThreads>(m, x, y, dot, ws, kLatChunkMin, kLatChunkMax);
    return RAMD_OK;
}
template int launch_csr_lat<double>(const ramd_mat_s*, const double*, double*, bool, CsrDotWs);
template int launch_csr_lat<float>(const ramd_mat_s*, const float*, float*, bool, CsrDotWs);

template <typename T>
int launch_cg_lat(const ramd_mat_s* m, const CgLatArgs<T>& a, CsrDotWs ws)
{
    if(m->lat_state != 1 || !m->lat_vals || !m->pat_id)
        RAMD_FAIL(RAMD_ERR_ARG, "launch_cg_lat: the matrix is not in lattice state 1");
    Backend&     b = backend();
    LatDims      g;
    const int    blocks = lat_geometry<kLatTX, kLatTY>(m, kLatChunkMin, kLatChunkMax, &g);
    const bool   coded  = a.count > 1;
    const size_t lds    = sizeof(T) * (size_t)(2 * (kLatTX + 2) * (kLatTY + 2) + g.npat * kLatSlotW + (coded ? a.count : 0));
    if(a.xmode != kCgXEach && a.xmode != kCgXDefer && a.xmode != kCgXBoth)
        RAMD_FAIL(RAMD_ERR_ARG, "launch_cg_lat: unknown x mode");
    // (kCgXEach has no slot for alpha: the kernel neither reads nor writes one)
    double* const alpha_out = a.xmode == kCgXDefer ? b.d_scalars + a.slot_alpha : nullptr;
#define GO(CODED, NTS, XM)                                                                                                      \
    hipLaunchKernelGGL((k_cg_lat<T, CODED, NTS, XM, kLatTX, kLatTY, kLatThreads>), dim3((unsigned)blocks), dim3(kLatThreads),   \
                       lds, b.cur, g, a.x, a.p_old, a.p_new, a.r, a.q, a.duni, a.table, a.count, a.codes, b.d_scalars,           \
                       a.slot_rho, a.slot_pq, a.slot_new, m->pat_id, (const T*)m->lat_vals, ws, a.slot_alpha, alpha_out)
#define GO_X(CODED, NTS)              \
    do                                \
    {                                 \
        if(a.xmode == kCgXDefer)      \
            GO(CODED, NTS, kCgXDefer); \
        else if(a.xmode == kCgXBoth)  \
            GO(CODED, NTS, kCgXBoth); \
        else                          \
            GO(CODED, NTS, kCgXEach); \
    } while(0)
    if(coded && a.nts)
        GO_X(true, true);
    else if(coded)
        GO_X(true, false);
    else if(a.nts)
        GO_X(false, true);
    else
        GO_X(false, false);
#undef GO_X
#undef GO
    return RAMD_OK;
}
template int launch_cg_lat<double>(const ramd_mat_s*, const CgLatArgs<double>&, CsrDotWs);
template int launch_cg_lat<float>(const ramd_mat_s*, const CgLatArgs<float>&, CsrDotWs);

} // namespace ramd
