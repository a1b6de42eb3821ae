// schwarz.hip -- the additive Schwarz preconditioners AS and RAS on gfx950: layout, restriction, prolongation and the direct
// sum of the diagonal blocks.
//
// Reference: src/solvers/preconditioners/preconditioner_as.cpp (Build :107-189, AS::Solve :238-272, RAS::Solve :342-373).
//
// With n rows, nb blocks, size = n / nb and the overlap ov, block b is the index range [pos_b, pos_b + len_b) of the operator:
//     pos_0 = 0, pos_b = b size - ov ;  len_b = size + ov (first and last block), size + 2 ov (the others)
// and rows nb size .. n - 1 belong to no block.  An apply restricts rhs to the nb ranges (split), solves the nb local systems
// (the caller's solvers) and puts the pieces together (join):
//     AS   x = 0 ; x[pos_b ...] = 1 x + 1 z_b for b ascending ; x *= w      (w: ones, 0.5 where the reference's loop put it)
//     RAS  x[b size ... (b + 1) size) = the piece of z_b that block b owns  (rows of no block are not written)
// The nb block systems are independent, so they can also be ONE system on the direct sum of the diagonal blocks: the pieces
// then lie behind one another in an "arena" of S = sum len_b elements, piece b at off_b = sum_{k < b} len_k, and the direct
// sum is an S x S CSR matrix assembled here (a rule of csr_filter.hpp).  Three forms of the vector work:
//   stepwise (form 0)  the reference's calls one by one: nb copies | Zeros, nb ScaleAddScale, PointWiseMult (RAS: nb copies)
//   fused    (form 1)  k_as_split / k_as_join on nb piece vectors, whose pointers travel by value (up to kAsMaxPieces;
//                      beyond that the stepwise calls)
//   stacked  (form 2)  the same two kernels on the arena, and the direct sum as the one local operator
// form -1 takes the stacked form (tools/schwarz_measure.py and profiles/schwarz.md hold the measurement; the class layer
// falls back to the fused form where the local solvers do not allow the direct sum).
// All three give the same bits: per element the join is (+0 + z_a) + z_b ... in ascending block order, times w, the
// roundings of the reference's sequence in its order (+0 + (-0) = +0 included).  The weight is computed from the row index;
// the stored weight vector exists for the stepwise form and for ramd_as_weights.
// Block of an arena element s: (s + ov) / (size + 2 ov); blocks that can cover row r: r / size - 1, r / size, r / size + 1
// (ov <= size): arithmetic only, no table per row.  Indices are 64-bit: S can exceed n.
#include "csr_filter.hpp"
#include "device_utils.hpp"
#include "matrix_impl.hpp"

#include <string>
#include <vector>

struct ramd_as_s
{
    int                     dtype = RAMD_F64;
    int                     n = 0, nb = 0, ov = 0, size = 0;
    int                     restricted = 0, form = 0;
    int64_t                 S = 0, stacked_nnz = 0;
    std::vector<int>        pos, sizes;
    std::vector<int64_t>    off; // [nb + 1]
    ramd_vec_t              weight = nullptr;
    std::vector<ramd_mat_t> locals; // what ramd_as_local has not handed out yet (nb blocks, or the direct sum alone)
    void                    release()
    {
        if(weight)
            (void)ramd_vec_destroy(weight);
        weight = nullptr;
        for(ramd_mat_t m : locals)
            if(m)
                (void)ramd_mat_destroy(m);
        locals.clear();
    }
};

namespace ramd
{

constexpr int kAsMaxPieces = 64; // piece pointers that travel as a kernel argument (512 bytes)

struct AsGeom
{
    int64_t n, S;
    int     nb, size, ov;
};
template <typename T>
struct AsPieces
{
    T* p[kAsMaxPieces];
};

typedef float v2f32 __attribute__((ext_vector_type(2)));
template <typename T>
struct Pair;
template <>
struct Pair<double>
{
    using type = v2f64;
};
template <>
struct Pair<float>
{
    using type = v2f32;
};

__host__ __device__ __forceinline__ int64_t as_pos(const AsGeom& g, int b)
{
    return b == 0 ? 0 : (int64_t)b * g.size - g.ov;
}
__host__ __device__ __forceinline__ int64_t as_len(const AsGeom& g, int b)
{
    return (int64_t)g.size + (b > 0 ? g.ov : 0) + (b < g.nb - 1 ? g.ov : 0);
}
__host__ __device__ __forceinline__ int64_t as_off(const AsGeom& g, int b)
{
    return b == 0 ? 0 : (int64_t)b * g.size + (int64_t)(2 * b - 1) * g.ov;
}
__host__ __device__ __forceinline__ int as_block_of(const AsGeom& g, int64_t s) // s < S
{
    return (int)((s + g.ov) / ((int64_t)g.size + 2 * (int64_t)g.ov));
}

// where piece b, element l lives: the arena (one array) or the b-th piece vector
template <typename T, bool PIECES>
__device__ __forceinline__ T* as_slot(const AsGeom& g, T* arena, const AsPieces<T>& pc, int b, int64_t l)
{
    if(PIECES)
        return pc.p[b] + l;
    return arena + as_off(g, b) + l;
}

// restriction: r[off_b + l] = rhs[pos_b + l].  A thread takes two consecutive arena elements; where both lie in one block
// and the source index is even too, they move as one 16-byte (fp32: 8-byte) packet, the block edges element by element
template <typename T, bool PIECES>
__global__ __launch_bounds__(kBlock) void k_as_split(AsGeom g, const T* __restrict__ rhs, T* __restrict__ arena, AsPieces<T> pc)
{
    typedef typename Pair<T>::type P2;
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * t < g.S; t += gsz)
    {
        const int64_t s0 = 2 * t;
        const int     b0 = as_block_of(g, s0);
        const int64_t l0 = s0 - as_off(g, b0), src0 = as_pos(g, b0) + l0;
        if(s0 + 1 < g.S && l0 + 1 < as_len(g, b0) && (src0 & 1) == 0 && (PIECES ? (l0 & 1) == 0 : true))
        {
            const P2 v                                                = *reinterpret_cast<const P2*>(rhs + src0);
            *reinterpret_cast<P2*>(as_slot<T, PIECES>(g, arena, pc, b0, l0)) = v;
            continue;
        }
        *as_slot<T, PIECES>(g, arena, pc, b0, l0) = rhs[src0];
        if(s0 + 1 < g.S)
        {
            const int     b1                             = as_block_of(g, s0 + 1);
            const int64_t l1                             = s0 + 1 - as_off(g, b1);
            *as_slot<T, PIECES>(g, arena, pc, b1, l1) = rhs[as_pos(g, b1) + l1];
        }
    }
}

// the value of row r of x after the join (AS), r < nb size: the covering blocks in ascending order, then the weight
template <typename T, bool PIECES>
__device__ __forceinline__ T as_row(const AsGeom& g, const T* arena, const AsPieces<T>& pc, int64_t r)
{
    const int k   = (int)(r / g.size);
    T         acc = (T)0;
#pragma unroll
    for(int d = -1; d <= 1; ++d)
    {
        const int b = k + d;
        if(b < 0 || b >= g.nb)
            continue;
        const int64_t p = as_pos(g, b);
        if(r >= p && r < p + as_len(g, b))
            acc = (T)1 * acc + (T)1 * *as_slot<T, PIECES>(g, const_cast<T*>(arena), pc, b, r - p);
    }
    // (preconditioner_as.cpp:140-154) 0.5 on [j size - ov, j size) for j = 1 .. nb - 1 and on [size, size + ov)
    const int64_t m    = r - (int64_t)k * g.size;
    const bool    half = g.nb >= 2 && ((k + 1 <= g.nb - 1 && m >= (int64_t)g.size - g.ov) || (r >= g.size && r < (int64_t)g.size + g.ov));
    return acc * (half ? (T)0.5 : (T)1);
}

// prolongation: one pass over the rows of x, every row written at most once, x never read.  AS: rows of no block get +0.
// RAS: the entry of the block that owns the row, rows of no block are left alone.  Two rows per thread, stored as a pair
// where both are written
template <typename T, bool PIECES, bool RESTRICTED>
__global__ __launch_bounds__(kBlock) void k_as_join(AsGeom g, const T* __restrict__ arena, AsPieces<T> pc, T* __restrict__ x)
{
    typedef typename Pair<T>::type P2;
    const int64_t gsz     = (int64_t)gridDim.x * blockDim.x;
    const int64_t covered = (int64_t)g.nb * g.size;
    for(int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; 2 * t < g.n; t += gsz)
    {
        const int64_t r0 = 2 * t;
        T             v[2];
        bool          w[2];
#pragma unroll
        for(int e = 0; e < 2; ++e)
        {
            const int64_t r = r0 + e;
            w[e]            = r < g.n && (!RESTRICTED || r < covered);
            v[e]            = (T)0;
            if(r < covered)
            {
                if(RESTRICTED)
                {
                    const int k = (int)(r / g.size);
                    v[e]        = *as_slot<T, PIECES>(g, const_cast<T*>(arena), pc, k, r - as_pos(g, k));
                }
                else
                    v[e] = as_row<T, PIECES>(g, arena, pc, r);
            }
        }
        if(w[0] && w[1])
        {
            P2 o;
            o[0]                             = v[0];
            o[1]                             = v[1];
            *reinterpret_cast<P2*>(x + r0) = o;
        }
        else if(w[0])
            x[r0] = v[0];
    }
}

// direct sum, as a rule of csr_filter.hpp: arena row s = off_b + l is source row pos_b + l; an entry stays if its column lies
// in the block's range and moves to col - pos_b + off_b; order within a row unchanged (the rule of ExtractSubMatrix)
struct AsSumRule
{
    static constexpr bool kRowsOnce = false; // (rows of an overlap belong to two blocks)
    AsGeom                g;
    struct Row
    {
        int64_t src, p, e, o; // source row; the block's range [p, e) of the operator and its offset in the arena
    };
    __device__ Row row(int64_t s) const
    {
        const int     b = as_block_of(g, s);
        const int64_t p = as_pos(g, b), o = as_off(g, b);
        return Row{p + s - o, p, p + as_len(g, b), o};
    }
    template <typename T>
    __device__ bool keep(const Row& r, int col, T) const { return col >= r.p && col < r.e; }
    __device__ int  col(const Row& r, int col) const { return (int)(col - r.p + r.o); }
};

namespace
{

AsGeom as_geom(const ramd_as_s* h)
{
    AsGeom g;
    g.n    = h->n;
    g.S    = h->S;
    g.nb   = h->nb;
    g.size = h->size;
    g.ov   = h->ov;
    return g;
}

int as_fail_layout(const std::string& what)
{
    RAMD_FAIL(RAMD_ERR_ARG, "AS: " + what);
}

// the direct sum of the diagonal blocks of the narrow CSR matrix A
int as_direct_sum(ramd_as_s* h, const ramd_mat_s* A, ramd_mat_t out)
{
    const AsGeom g = as_geom(h);
    if(g.S > kWideMaxRows)
        RAMD_FAIL(RAMD_ERR_UNSUPPORTED, "AS: the direct sum of the blocks has more rows than a matrix holds");
    const int s = csr_filter("AS", "the direct sum of the blocks", AsSumRule{g}, A, A->rp, (int)g.S, (int)g.S, out);
    if(s == RAMD_ERR_HIP)
        RAMD_FAIL(s, "AS: assembling the direct sum of the blocks failed");
    if(s == RAMD_OK)
        h->stacked_nnz = out->nnz;
    return s;
}

// the weights as the reference's loop writes them (preconditioner_as.cpp:133-156), on the host, copied over once
template <typename T>
int as_weights(ramd_as_s* h)
{
    std::vector<T> w((size_t)h->n, (T)1);
    for(int i = 0; i < h->nb; ++i)
        for(int j = 0; j < h->ov; ++j)
        {
            if(i != 0)
                w[(size_t)h->pos[i] + j] = (T)0.5;
            if(i != h->nb - 1)
                w[(size_t)h->pos[i] + h->size + j] = (T)0.5;
        }
    RAMD_TRY(ramd_vec_create(h->dtype, &h->weight));
    RAMD_TRY(ramd_vec_allocate(h->weight, h->n));
    return ramd_vec_copy_from_host(h->weight, w.data());
}

int as_check_vec(const ramd_as_s* h, ramd_vec_t v, int64_t n, const char* what)
{
    if(!v || v->dtype != h->dtype || v->n != n)
        RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": vector size / type mismatch");
    return RAMD_OK;
}
int as_check_pieces(const ramd_as_s* h, const ramd_vec_t* p, int nb, ramd_vec_t other, const char* what)
{
    if(!p || nb != h->nb)
        RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": one piece vector per block expected");
    for(int i = 0; i < nb; ++i)
    {
        RAMD_TRY(as_check_vec(h, p[i], h->sizes[i], what));
        if(p[i] == other)
            RAMD_FAIL(RAMD_ERR_ARG, std::string(what) + ": a piece must not be the full-length vector");
    }
    return RAMD_OK;
}

template <typename T>
int as_split_t(const ramd_as_s* h, ramd_vec_t rhs, T* arena, const ramd_vec_t* pieces)
{
    const AsGeom g = as_geom(h);
    AsPieces<T>  pc;
    for(int i = 0; i < kAsMaxPieces; ++i)
        pc.p[i] = pieces && i < h->nb ? (T*)pieces[i]->d : nullptr;
    const int grid = ew_grid((g.S + 1) / 2);
    if(pieces)
        hipLaunchKernelGGL((k_as_split<T, true>), dim3(grid), dim3(kBlock), 0, backend().cur, g, (const T*)rhs->d, (T*)nullptr, pc);
    else
        hipLaunchKernelGGL((k_as_split<T, false>), dim3(grid), dim3(kBlock), 0, backend().cur, g, (const T*)rhs->d, arena, pc);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

template <typename T>
int as_join_t(const ramd_as_s* h, const T* arena, const ramd_vec_t* pieces, ramd_vec_t x)
{
    const AsGeom g = as_geom(h);
    AsPieces<T>  pc;
    for(int i = 0; i < kAsMaxPieces; ++i)
        pc.p[i] = pieces && i < h->nb ? (T*)pieces[i]->d : nullptr;
    const dim3 grid(ew_grid((g.n + 1) / 2)), block(kBlock);
    hipStream_t st = backend().cur;
    if(pieces && h->restricted)
        hipLaunchKernelGGL((k_as_join<T, true, true>), grid, block, 0, st, g, (const T*)nullptr, pc, (T*)x->d);
    else if(pieces)
        hipLaunchKernelGGL((k_as_join<T, true, false>), grid, block, 0, st, g, (const T*)nullptr, pc, (T*)x->d);
    else if(h->restricted)
        hipLaunchKernelGGL((k_as_join<T, false, true>), grid, block, 0, st, g, arena, pc, (T*)x->d);
    else
        hipLaunchKernelGGL((k_as_join<T, false, false>), grid, block, 0, st, g, arena, pc, (T*)x->d);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

} // namespace
} // namespace ramd

using namespace ramd;

extern "C" {

int ramd_as_layout(int64_t n, int nb, int overlap, int* pos_out, int* sizes_out)
{
    if(nb < 1)
        return as_fail_layout("the number of blocks must be at least 1 (got " + std::to_string(nb) + ")");
    if(overlap < 0)
        return as_fail_layout("the overlap must not be negative (got " + std::to_string(overlap) + ")");
    if(n < 0 || n > INT32_MAX)
        return as_fail_layout("the row count is out of range");
    if(n / nb < 1)
        return as_fail_layout("fewer rows than blocks (" + std::to_string(n) + " rows, " + std::to_string(nb) + " blocks)");
    const int size = (int)(n / nb);
    if(nb == 1 && overlap > 0)
        return as_fail_layout("one block with an overlap would overrun the matrix (use overlap 0)");
    if(nb >= 2 && overlap > size)
        return as_fail_layout("the overlap (" + std::to_string(overlap) + ") is larger than a block (" + std::to_string(size)
                              + " rows): the second block would start before row 0");
    if(!pos_out || !sizes_out)
        return as_fail_layout("null result pointer");
    // (preconditioner_as.cpp:117-131)
    int offset = 0;
    for(int i = 0; i < nb; ++i)
    {
        pos_out[i] = offset - overlap;
        offset += size;
        sizes_out[i] = size + 2 * overlap;
    }
    pos_out[0]        = 0;
    sizes_out[0]      = size + overlap;
    sizes_out[nb - 1] = size + overlap;
    return RAMD_OK;
}

int ramd_as_build(ramd_mat_t op, int nb, int overlap, int restricted, int form, ramd_as_t* out)
{
    RAMD_NARROW_ONLY(op);
    if(!op || !out || form < -1 || form > 2)
        RAMD_FAIL(RAMD_ERR_ARG, "AS: bad arguments (form is -1 auto, 0 stepwise, 1 fused, 2 stacked)");
    if(op->dtype != RAMD_F64 && op->dtype != RAMD_F32)
        RAMD_FAIL(RAMD_ERR_ARG, "AS: a real operator expected");
    if(op->nrow != op->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "AS: the operator is not square");
    std::vector<int> pos((size_t)(nb > 0 ? nb : 1)), sizes((size_t)(nb > 0 ? nb : 1));
    RAMD_TRY(ramd_as_layout(op->nrow, nb, overlap, pos.data(), sizes.data()));
    ramd_as_s* h  = new ramd_as_s;
    h->dtype      = op->dtype;
    h->n          = op->nrow;
    h->nb         = nb;
    h->ov         = overlap;
    h->size       = op->nrow / nb;
    h->restricted = restricted ? 1 : 0;
    h->form       = form == -1 ? 2 : form;
    h->pos        = pos;
    h->sizes      = sizes;
    h->off.assign((size_t)nb + 1, 0);
    for(int i = 0; i < nb; ++i)
        h->off[(size_t)i + 1] = h->off[(size_t)i] + sizes[(size_t)i];
    h->S = h->off[(size_t)nb];
    ramd_mat_t A = op, copy = nullptr;
    int        s = RAMD_OK;
    if(op->format != RAMD_CSR)
    {
        s = ramd_mat_clone(op, &copy);
        if(s == RAMD_OK)
            s = ramd_mat_convert(copy, RAMD_CSR);
        A = copy;
    }
    if(s == RAMD_OK)
        s = h->dtype == RAMD_F64 ? as_weights<double>(h) : as_weights<float>(h);
    if(s == RAMD_OK && h->form == 2)
    {
        ramd_mat_t m = nullptr;
        s            = ramd_mat_create(h->dtype, &m);
        if(s == RAMD_OK)
        {
            h->locals.push_back(m);
            s = as_direct_sum(h, A, m);
        }
    }
    else if(s == RAMD_OK)
        for(int i = 0; i < nb && s == RAMD_OK; ++i)
        {
            ramd_mat_t m = nullptr;
            s            = ramd_mat_create(h->dtype, &m);
            if(s == RAMD_OK)
            {
                h->locals.push_back(m);
                s = ramd_mat_extract_submatrix(A, pos[(size_t)i], pos[(size_t)i], sizes[(size_t)i], sizes[(size_t)i], m);
            }
        }
    if(copy)
        (void)ramd_mat_destroy(copy);
    if(s != RAMD_OK)
    {
        h->release();
        delete h;
        return s;
    }
    *out = h;
    return RAMD_OK;
}

int ramd_as_local(ramd_as_t h, int block, ramd_mat_t* out)
{
    if(!h || !out || block < 0 || block >= (int)h->locals.size())
        RAMD_FAIL(RAMD_ERR_ARG, "as_local: bad arguments (the stacked form has the one local operator 0)");
    if(!h->locals[(size_t)block])
        RAMD_FAIL(RAMD_ERR_STATE, "as_local: this local operator was handed out already");
    *out                      = h->locals[(size_t)block];
    h->locals[(size_t)block] = nullptr;
    return RAMD_OK;
}

int ramd_as_split(ramd_as_t h, ramd_vec_t rhs, ramd_vec_t r)
{
    if(!h || rhs == r)
        RAMD_FAIL(RAMD_ERR_ARG, "as_split: bad arguments (rhs and r must be two vectors)");
    RAMD_TRY(as_check_vec(h, rhs, h->n, "as_split"));
    RAMD_TRY(as_check_vec(h, r, h->S, "as_split"));
    return h->dtype == RAMD_F64 ? as_split_t<double>(h, rhs, (double*)r->d, nullptr) : as_split_t<float>(h, rhs, (float*)r->d, nullptr);
}

int ramd_as_split_v(ramd_as_t h, ramd_vec_t rhs, const ramd_vec_t* r, int nb)
{
    if(!h)
        RAMD_FAIL(RAMD_ERR_ARG, "as_split_v: null plan");
    RAMD_TRY(as_check_vec(h, rhs, h->n, "as_split_v"));
    RAMD_TRY(as_check_pieces(h, r, nb, rhs, "as_split_v"));
    if(h->form == 0 || nb > kAsMaxPieces) // (preconditioner_as.cpp:246-249)
    {
        for(int i = 0; i < nb; ++i)
            RAMD_TRY(ramd_vec_copy_from_offset(r[i], rhs, h->pos[(size_t)i], 0, h->sizes[(size_t)i]));
        return RAMD_OK;
    }
    return h->dtype == RAMD_F64 ? as_split_t<double>(h, rhs, nullptr, r) : as_split_t<float>(h, rhs, nullptr, r);
}

int ramd_as_join(ramd_as_t h, ramd_vec_t z, ramd_vec_t x)
{
    if(!h || z == x)
        RAMD_FAIL(RAMD_ERR_ARG, "as_join: bad arguments (z and x must be two vectors)");
    RAMD_TRY(as_check_vec(h, z, h->S, "as_join"));
    RAMD_TRY(as_check_vec(h, x, h->n, "as_join"));
    return h->dtype == RAMD_F64 ? as_join_t<double>(h, (const double*)z->d, nullptr, x) : as_join_t<float>(h, (const float*)z->d, nullptr, x);
}

int ramd_as_join_v(ramd_as_t h, const ramd_vec_t* z, int nb, ramd_vec_t x)
{
    if(!h)
        RAMD_FAIL(RAMD_ERR_ARG, "as_join_v: null plan");
    RAMD_TRY(as_check_vec(h, x, h->n, "as_join_v"));
    RAMD_TRY(as_check_pieces(h, z, nb, x, "as_join_v"));
    if(h->form == 0 || nb > kAsMaxPieces)
    {
        if(h->restricted) // (preconditioner_as.cpp:363-370)
        {
            int64_t z_offset = 0;
            for(int i = 0; i < nb; ++i)
            {
                RAMD_TRY(ramd_vec_copy_from_offset(x, z[i], z_offset, h->pos[(size_t)i] + z_offset, h->size));
                z_offset = h->ov;
            }
            return RAMD_OK;
        }
        RAMD_TRY(ramd_vec_zeros(x)); // (:258-269)
        for(int i = 0; i < nb; ++i)
            RAMD_TRY(ramd_vec_scale_add_scale_offset(x, 1.0, z[i], 1.0, 0, h->pos[(size_t)i], h->sizes[(size_t)i]));
        return ramd_vec_pointwise_mult(x, h->weight);
    }
    return h->dtype == RAMD_F64 ? as_join_t<double>(h, nullptr, z, x) : as_join_t<float>(h, nullptr, z, x);
}

int ramd_as_weights(ramd_as_t h, ramd_vec_t w)
{
    if(!h || !w || w->dtype != h->dtype)
        RAMD_FAIL(RAMD_ERR_ARG, "as_weights: a vector of the plan's type expected");
    return ramd_vec_copy_from(w, h->weight);
}

int ramd_as_info(ramd_as_t h, int64_t* out8)
{
    if(!h || !out8)
        RAMD_FAIL(RAMD_ERR_ARG, "as_info: bad arguments");
    out8[0] = h->form;
    out8[1] = h->nb;
    out8[2] = h->ov;
    out8[3] = h->size;
    out8[4] = h->S;
    out8[5] = (int64_t)h->n - (int64_t)h->nb * h->size;
    out8[6] = h->stacked_nnz;
    out8[7] = h->restricted;
    return RAMD_OK;
}

int ramd_as_piece_cap(void)
{
    return kAsMaxPieces;
}

int ramd_as_destroy(ramd_as_t h)
{
    if(h)
    {
        h->release();
        delete h;
    }
    return RAMD_OK;
}

} // extern "C"
