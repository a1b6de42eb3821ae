// spmv_lattice.hpp -- lattice form of the value-pattern CSR product (spmv_lattice.hip), dispatched by launch_csr_patv (spmv.hip).
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

} // namespace ramd
