// spmv_lattice.hpp -- lattice form of the value-pattern CSR product (spmv_lattice.hip), dispatched by launch_csr (spmv.hip).
#pragma once

#include "matrix_impl.hpp"

namespace ramd
{

// slots of a row of a lattice operator, in ascending column order: -nx ny, -nx, -1, 0, +1, +nx, +nx ny
constexpr int kLatSlots = 7;
// ramd_mat_s::lat_vals holds kLatSlotW values per dictionary entry: the seven slots' values and, as the eighth, the entry's
// mask of present slots (bit s = slot s) as a number
constexpr int kLatSlotW = 8;

// y = A x of a matrix in lattice state 1 (csr_analyse_lattice), dot: with the per-wave partials of <dotv or x, y> in
// ws.part1[row / 64] -- the places and the grouping of k_csr_patv, results identical bit for bit.  The caller brackets the
// launch and reduces the partials.
template <typename T>
int launch_csr_lat(const ramd_mat_s* m, const T* x, T* y, bool dot, CsrDotWs ws);

// CG + Jacobi: the direction update and the product that follows it as one launch (k_cg_lat, spmv_lattice.hip)
//   p_new = beta p_old + d r ; x += alpha p_old ; q = A p_new ; partials of <p_new, q> in ws.part1
// alpha = s[slot_rho] / s[slot_pq], beta = s[slot_new] / s[slot_rho], d from the coded form of the inverse diagonal (count 1:
// duni; more: table / codes).  x, p_new and q are written; none of the five vectors may be another one.
// xmode, the x update of two launches done by the second (the values of RAMD_CG_X_* in rocalution_amd.h):
//   kCgXEach   as above
//   kCgXDefer  x is not touched; s[slot_alpha] = alpha
//   kCgXBoth   x = (x + s[slot_alpha] * p_new as found) + alpha p_old; p_new must hold, on entry, the p_old of the deferring
//              launch -- which it does where the two buffers of p swap roles from launch to launch
constexpr int kCgXEach = 0, kCgXDefer = 1, kCgXBoth = 2;
template <typename T>
struct CgLatArgs
{
    T*                   x;
    const T*             p_old;
    T*                   p_new;
    const T*             r;
    T*                   q;
    T                    duni;
    const T*             table;
    int                  count;
    const unsigned char* codes;
    int                  slot_rho, slot_pq, slot_new;
    bool                 nts; // non-temporal stores of x and p_new
    int                  xmode, slot_alpha; // (slot_alpha: kCgXDefer and kCgXBoth only)
};
template <typename T>
int launch_cg_lat(const ramd_mat_s* m, const CgLatArgs<T>& a, CsrDotWs ws);

// spmv.hip: whether ramd_fused_apply_dot of this matrix is k_csr_lat as things stand -- lattice state 1, value state 1, 32-bit
// row offsets, the process' switches admit the kernel and the size (no analysis is run) -- and RAMD_CG_LATDIR is not 0; and
// the launch with its bracket and the reduction of the partials into s[a.slot_pq]
bool csr_cg_lat_ready(const ramd_mat_s* m);
template <typename T>
int csr_cg_lat(const ramd_mat_s* m, const CgLatArgs<T>& a);

} // namespace ramd
