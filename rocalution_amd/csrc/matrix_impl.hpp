// matrix_impl.hpp -- internal (non-ABI) declarations shared by the .hip translation units.
#pragma once

#include "common.hpp"
#include "spmv_pick.hpp"

#include <type_traits>

namespace ramd
{

size_t val_size(int dtype);
void   mat_free_csr(ramd_mat_s* m);
void   mat_free_ell(ramd_mat_s* m);
void   mat_free_coo(ramd_mat_s* m);
void   mat_free_bcsr(ramd_mat_s* m);
void   mat_free_dia(ramd_mat_s* m);
void   mat_free_mcsr(ramd_mat_s* m);
void   mat_free_analysis(ramd_mat_s* m);
void   mat_format_changed(ramd_mat_s* m); // CSR <-> ELL / HYB / COO: mat_free_analysis, but the far-band distance stays
void   mat_values_changed(ramd_mat_s* m); // val was (or is about to be) written in place: the value dictionary is analysed again
int    mat_alloc_csr(ramd_mat_s* m, int nrow, int ncol, int64_t nnz);
// wide CSR (64-bit row offsets, matrix.hip): allocate rp64 / ci / val with rp == nullptr; derive the kernels' compact form
// (blk_rp64, row_off) once rp64 is filled
// (rows: the kernels form block * 256 + thread as an int before they compare it with nrow)
constexpr int kWideMaxRows = 2147483647 - 256;
int    mat_alloc_csr_wide(ramd_mat_s* m, int nrow, int ncol, int64_t nnz);
int    mat_wide_finish(ramd_mat_s* m);
int    mat_narrow_offsets(const int64_t* in, int* out, int64_t n); // out[i] = (int)in[i], the caller knows that they fit
inline bool mat_is_wide(const ramd_mat_s* m)
{
    return m->rp64 != nullptr;
}

// spmv.hip: detect a far band (3-D stencil plane distance) for the band-aware row-block traversal
int csr_analyse_band(ramd_mat_s* m);
int csr_analyse_groups(ramd_mat_s* m);
int csr_analyse_pattern(ramd_mat_s* m); // the row-pattern dictionary (narrow and wide CSR)
int csr_analyse_values(ramd_mat_s* m); // ... and the values of its entries, where they are a function of the pattern
int csr_analyse_lattice(ramd_mat_s* m); // ... and whether the dictionary is that of a 5- / 7-point operator on an nx x ny x nz lattice
int csr_analyse_shift(ramd_mat_s* m); // rows that are their predecessor shifted by one column (stencils): ramd_mat_s::shift_rows
// row patterns (spmv.hip): rows whose column offsets col - row coincide share a dictionary entry of kPatMaxW slots
constexpr int kPatMaxW = 28; // longest row a pattern may have (round 6: the 27 entries of the reference's own 3-D operator; 16 before)
constexpr int kPatMax  = 64; // dictionary entries
static_assert(kPatMaxW == kPickPatMaxW && kPatMax == kPickPatMax, "spmv_pick.hpp restates these");
constexpr int kPatEnd  = -2147483647 - 1; // dictionary entry of an ELL slot that holds no column (col < 0)
// x tiles of a structured CSR product (spmv.hip, k_csr_xl): the distinct column offsets of the dictionary fall into a few
// clusters; a 256-row block needs, per cluster, ONE contiguous piece of x -- loaded into LDS with 16-byte packets
constexpr int kXlSegs = 8; // clusters
struct XlSegs
{
    int nseg;
    int omin[kXlSegs]; // first element of the piece relative to the block's first row (a multiple of the packet size)
    int npk[kXlSegs]; // 16-byte packets of the piece
    int base[kXlSegs]; // where the piece starts in the LDS area (elements)
    int total; // elements of the LDS area in use (a multiple of the packet size)
};
// rows sharing the column list of the row before them (FE matrices: the unknowns of one mesh node): k_csr_tr<GRP>
struct CsrGroups
{
    const int*           lead; // [nrow] entry offset from a row's entries to its group leader's (<= 0)
    const unsigned char* need; // [nnz / 4] column packets that have to be read
};
// workspace of the epilogues of the CSR products (csr_row_epilogue, wave_rows.hpp): fused <x, y>, Jacobi sweep
struct CsrDotWs
{
    double*     part1; // [4 * nblk] one partial per wave
    const void* dotv; // the dot runs against this vector (nullptr: against x)
    const void* jdinv; // MODE 2 (Jacobi sweep): inverse diagonal and right-hand side
    const void* jrhs;
};
struct CsrPattern
{
    const unsigned char* id; // [nrow]
    const int*           dict; // [n * kPatMaxW]
    int                  n, w;
};
// the same analysis for a wave-sliced ELL (slices of 64 rows, column-major inside a slice: the MC-SGS sweeps); on success
// *state = 1 and *id / *dict are device arrays the caller owns, else *state = -1
int sell_analyse_pattern(int nrow, const int* slice_off, const int* ecol, int* state, int* n, unsigned char** id, int** dict);

// backend.hip: optional HIP-event bracket around every SpMV launch (bench.py roofline leg)
void prof_spmv_begin();
void prof_spmv_end();
void prof_begin(int channel, hipStream_t s); // s == nullptr: the current stream
void prof_end(int channel, hipStream_t s);
void prof_count(int channel); // count an occurrence without timing it

// trisolve.hip
void tri_release(ramd_mat_s* m);
int  mat_transpose(const ramd_mat_s* m, ramd_mat_s* t); // t = m^T, rows sorted

// matrix_algebra.hip: *out = new matrix with the (row-sorted) pattern of a^q, SymbolicPower(q)
int mat_symbolic_power(const ramd_mat_s* a, int q, ramd_mat_s** out);

// blocksched.hip: hyperplane order of the row blocks for the natural-order sync-free sweeps (nullptr: natural)
int block_schedule(const ramd_mat_s* m, bool lower, int** order_out);
// ... and the wave units (<= 64 consecutive sweep rows that belong together) of the sweeps with in-wave register resolution
// (trisolve.hip), with their order by level of the unit graph, all computed on the device
struct UnitPlan
{
    int  nunits = 0;
    int* ustart = nullptr; // [nunits + 1] first sweep row of every unit
    int* order  = nullptr; // [nunits] or nullptr: natural order
    void release();
};
struct UnitView // (kernel argument)
{
    const int* ustart;
    const int* order;
    int        nunits;
};
inline UnitView unit_view(const UnitPlan& p)
{
    return UnitView{p.ustart, p.order, p.nunits};
}
int unit_schedule(const ramd_mat_s* m, bool lower, UnitPlan* out);

// coloring.hip: device greedy colouring; RAMD_ERR_UNSUPPORTED -> caller runs the host sweep
int multicoloring_device(const ramd_mat_s* m, int* num_colors, int* size_colors, ramd_vec_s* perm);

// spmv.hip
template <typename T>
int mat_apply_impl(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar);
template <typename T>
int mat_apply_dot_impl(const ramd_mat_s* m, const T* x, T* y, int slot, const T* dotv = nullptr);
template <typename T>
int mat_jacobi_sweep_impl(const ramd_mat_s* m, const T* dinv, const T* rhs, const T* x, T* xnew, T omega);
template <typename T>
int mat_apply_add_dot_impl(const ramd_mat_s* m, const T* x, T* y, T scalar, const T* p, int slot);
// spmv_wide.hip: the launch of k_csr_wide<use_pat>, the kernel of a CSR matrix with 64-bit row offsets (launch_csr, spmv.hip,
// has picked it and owns the workspace ws; mode 0: y = A x, 1: y += scalar A x, 2: Jacobi sweep; dot: fused <dotv or x, y>)
template <typename T>
int launch_csr_wide(const ramd_mat_s* m, bool use_pat, const T* x, T* y, int mode, bool dot, T scalar, const CsrDotWs& ws);

// spmv.hip: pick the kernel of a product of a CSR / ELL / HYB matrix (spmv_pick.hpp), running the analyses the choice waits for
int spmv_prepare(const ramd_mat_s* m, int mode, bool dot, CsrPick* pick);
// the workspace of a fused dot, kept with the matrix: one partial per wave of nblk workgroups
int mat_dot_partials(const ramd_mat_s* m, int nblk, double** part1);
// f(MODE, DOT) as integral constants for a product's runtime (mode, dot): (0, dot) for mode 0, (2, false) for mode 2 where the
// format has a sweep (MODE2), else (1, false) -- as the cascades this replaces, a format without MODE2 takes mode 2 for mode 1.
// Every format instantiates its kernels for these and no other pairs
template <bool MODE2, typename F>
inline void with_mode_dot(int mode, bool dot, F&& f)
{
    if(mode == 0 && dot)
        f(std::integral_constant<int, 0>(), std::true_type());
    else if(mode == 0)
        f(std::integral_constant<int, 0>(), std::false_type());
    else if constexpr(MODE2)
        mode == 2 ? f(std::integral_constant<int, 2>(), std::false_type()) : f(std::integral_constant<int, 1>(), std::false_type());
    else
        f(std::integral_constant<int, 1>(), std::false_type());
}

// bcsr.hip: the products of a BCSR matrix (mode 0: y = A x, 1: y += scalar * (A x); dot: fused <dotv or x, y>, mode 0 only),
// and BCSR -> CSR in place (ramd_mat_convert)
template <typename T>
int launch_bcsr(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv = nullptr);
int bcsr_to_csr(ramd_mat_s* m);

// dia.hip: the products of a DIA matrix (mode 0: y = A x, 1: y += (scalar * a) * x diagonal by diagonal; dot: fused
// <dotv or x, y>, mode 0 only), and CSR <-> DIA in place (ramd_mat_convert)
template <typename T>
int launch_dia(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv = nullptr);
int csr_to_dia(ramd_mat_s* m);
int dia_to_csr(ramd_mat_s* m);

// mcsr.hip: the products of an MCSR matrix (mode 0: y = A x, 1: y += (scalar * a) * x entry by entry, both starting with the
// diagonal; dot: fused <dotv or x, y>, mode 0 only), CSR <-> MCSR in place (ramd_mat_convert), and the (inverse) diagonal
// val[0 .. nrow) into d
template <typename T>
int launch_mcsr(const ramd_mat_s* m, const T* x, T* y, int mode, T scalar, bool dot, int slot, const T* dotv = nullptr);
int csr_to_mcsr(ramd_mat_s* m);
int mcsr_to_csr(ramd_mat_s* m);
int mcsr_extract_diag(const ramd_mat_s* m, void* d, bool inv);

// vector.hip: scalars[slot] = sum(a[0..n)) in one launch, fixed order
int reduce_sum_to_slot(const double* a, int64_t n, int slot);

// scan.hip: out[i] = sum_{k<i} in[k] for i < n (in and out may alias); int32 sums
int device_exclusive_scan(const int* in, int* out, int64_t n);
// the same with 64-bit sums: out[i] = sum_{k<i} in[k] as int64
int device_exclusive_scan64(const int* in, int64_t* out, int64_t n);
// order_out = indices 0..n-1 sorted by keys (0 <= key <= max_key), stable
int device_stable_sort_by_key(const int* keys, int64_t n, int max_key, int* order_out);
// max over an int array -> host
int device_max_int(const int* in, int64_t n, int* result);
// *differ = 1 (device) where two device arrays of 32-bit words are not equal (values are compared as bits: -0.0 is not +0.0,
// NaNs by payload); left alone where they are equal.  One launch on the current stream; the caller checks hipGetLastError()
void dev_words_differ(const void* a, const void* b, int64_t nwords, int* differ);

} // namespace ramd
