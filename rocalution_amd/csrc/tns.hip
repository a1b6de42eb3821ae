// tns.hip -- the TNS preconditioner (truncated Neumann series) on gfx950.
//
// Reference: src/solvers/preconditioners/preconditioner_ai.cpp:476-713 (class TNS).  With K = strict_lower(A) D^-1 the
// operator is M^-1 = (I - K^T + K^T^2) D^-1 (I - K + K^2); the reference's implicit Solve (:685-701) is, step by step,
//     t1 = K r ; t2 = K t1 ; t1 = t1 + (-1) t2 ; x = r ; x = x + (-1) t1 ; x = x * dinv
//     t1 = K^T x ; t2 = K^T t1 ; x = 1 x + (-1) t1 + 1 t2
// over two stored matrices (K = ExtractL . DiagonalMatrixMultR, rounded once per entry, and its row-sorted transpose): four
// products and five vector kernels.  One plan object holds one of three forms here, all with the reference's arithmetic
// (rows summed left to right in storage order from 0, no FMA contraction, the element-wise expressions of host_vector.cpp):
//
//   matrix-free   nothing but dinv, a split position per row and one work vector is stored.  For a bitwise symmetric A with
//                 sorted rows (K^T)_ij = a_ij dinv_i for j > i, so both triangles are read from A's own ci / val:
//                 four launches of k_tns_tri<T, UPPER, STAGE>, a product formed as (a_ij * dinv_s) * v_j with s = j (lower)
//                 or i (upper); the second and the fourth launch carry the element-wise steps.  A wave owns 64 rows, stages
//                 their entries in LDS in passes of kTnsCap and lane = row walks its own triangle (the wave-private row
//                 walk of wave_rows.hpp); a pass that holds no entry of the triangle wanted is not loaded.  No workgroup
//                 waits for another.
//   stored        K and K^T built with the library's own primitives exactly as the reference does, applied with
//                 mat_apply_impl (so the row-pattern and value-pattern products serve them) and two element-wise
//                 kernels: six launches.  Serves every matrix (unsymmetric, unsorted, ELL / HYB operators).
//   explicit      Set(false) (:559-599): TNS_ = (K2^T D^-1) K2 with K2 = L^2 - (L - I) from MatrixMult / MatrixAdd /
//                 Transpose / DiagonalMatrixMultR in the reference's order; the apply is one product.
#include "device_utils.hpp"
#include "matrix_impl.hpp"
#include "wave_rows.hpp"

#include <string>

namespace ramd
{

constexpr int kTnsCap = 1024; // entries of a wave's LDS image per pass (12 KiB in fp64)
constexpr int kTnsGW  = 8; // gathers in flight per row and array

// UPPER = false: sum_i = sum_{j < i} (a_ij * dinv_j) * v_j   (a row of K v)
// UPPER = true : sum_i = sum_{j > i} (a_ij * dinv_i) * v_j   (a row of K^T v, A symmetric)
// STAGE 0: out_i = sum_i
// STAGE 1, lower: out_i = (r_i + (-1) * (v_i + (-1) * sum_i)) * dinv_i        (AddScale, CopyFrom, AddScale, PointWiseMult)
// STAGE 1, upper: out_i = 1 * out_i + (-1) * v_i + 1 * sum_i                  (ScaleAdd2; out is x, read at row i only)
// split[i]: position of the first entry of row i with col >= i
template <typename T, bool UPPER, int STAGE>
__global__ __launch_bounds__(kBlock) void k_tns_tri(int nrow, const int* __restrict__ rp, const int* __restrict__ split,
                                                    const int* __restrict__ ci, const T* __restrict__ val,
                                                    const T* __restrict__ dinv, const T* __restrict__ v, const T* __restrict__ r,
                                                    T* out)
{
    extern __shared__ __attribute__((aligned(16))) char tns_lds[];
    T*        sval_all = reinterpret_cast<T*>(tns_lds); // [4][kTnsCap]
    int*      scol_all = reinterpret_cast<int*>(tns_lds + sizeof(T) * 4 * kTnsCap); // [4][kTnsCap]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * kBlock + 64 * wave;
    if(row0 >= nrow) // (wave-uniform; the kernel has no workgroup barrier)
        return;
    const int  row   = row0 + lane;
    const bool live  = row < nrow;
    const int  start = rp[row0];
    const int  end   = rp[min(row0 + 64, nrow)];
    int        ts = end, te = end; // the row's triangle [ts, te); a lane behind the last row has none
    T          drow = (T)0;
    if(live)
    {
        const int sp = split[row];
        ts           = UPPER ? sp : rp[row];
        te           = UPPER ? rp[row + 1] : sp;
        drow         = dinv[row];
    }
    // the wave's base (wave_rows.hpp): rows and passes are offsets from it
    const int  a0 = start & ~3;
    const T*   vw = val + a0;
    const int* cw = ci + a0;
    const int  lts = ts - a0, lte = te - a0, lend = end - a0;
    T*         sv  = sval_all + wave * kTnsCap;
    int*       sc  = scol_all + wave * kTnsCap;
    T          sum = (T)0;
    struct Elems // what an entry gathers: v_j and the dinv of its product
    {
        T xv, ds;
    };
    for(int cb = 0; cb < lend; cb += kTnsCap)
    {
        const int lo = max(lts, cb), hi = min(lte, cb + kTnsCap);
        const int len = hi - lo;
        if(__ballot(len > 0) == 0ull) // nothing of the wanted triangle in this pass (the other triangle of a long row)
            continue;
        wave_stage_pass<T, kTnsCap, true>(cw, vw, cb, lend, lane, sc, sv);
        sum =wave_walk_pass<T, kTnsGW>(
            sv, lo - cb, len, sum,
            [&](int idx, int k, bool& ok) {
                const int col = sc[idx];
                if(UPPER) // (the stored diagonal entry, where there is one, sits at the split position)
                    ok = ok && col > row;
                return col;
            },
            [&](int col) { return Elems{v[col], UPPER ? drow : dinv[col]}; },
            [&](T s, T a, Elems g) {
                const T kij = a * g.ds; // K's entry, rounded as DiagonalMatrixMultR stores it
                return s + kij * g.xv;
            });
    }
    if(live)
    {
        if(STAGE == 0)
            out[row] = sum;
        else if(!UPPER)
        {
            const T u = v[row] + (T)(-1) * sum;
            const T y = r[row] + (T)(-1) * u;
            out[row]  = y * drow;
        }
        else
            out[row] = (T)1 * out[row] + (T)(-1) * v[row] + (T)1 * sum;
    }
}

// split[i] = first position of row i with col >= i; *unsorted = 1 where a row's columns are not strictly ascending
__global__ __launch_bounds__(kBlock) void k_tns_split(int nrow, const int* __restrict__ rp, const int* __restrict__ ci,
                                                      int* __restrict__ split, int* __restrict__ unsorted)
{
    const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
    for(int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nrow; i += gsz)
    {
        const int b = rp[i], e = rp[i + 1];
        int       sp = e;
        bool      bad = false;
        for(int j = b; j < e; ++j)
        {
            const int c = ci[j];
            if(sp == e && c >= (int)i)
                sp = j;
            if(j > b && ci[j - 1] >= c)
                bad = true;
        }
        split[i] = sp;
        if(bad)
            *unsorted = 1;
    }
}

// the element-wise steps of the stored form, a 16-byte packet per thread and a scalar tail
// EPI 0: x = (r + (-1) * (t1 + (-1) * t2)) * dinv      EPI 1: x = 1 * x + (-1) * t1 + 1 * t2
template <typename T, int EPI>
__global__ __launch_bounds__(kBlock) void k_tns_epilogue(int64_t n, T* __restrict__ x, const T* __restrict__ r,
                                                         const T* __restrict__ t1, const T* __restrict__ t2,
                                                         const T* __restrict__ dinv)
{
    using P         = typename Pack<T>::type;
    constexpr int N = Pack<T>::N;
    auto one        = [](T xi, T ri, T a, T b, T d) -> T {
        if(EPI == 0)
        {
            const T u = a + (T)(-1) * b;
            const T y = ri + (T)(-1) * u;
            return y * d;
        }
        return (T)1 * xi + (T)(-1) * a + (T)1 * b;
    };
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if((i + 1) * N <= n)
    {
        P px = EPI == 1 ? reinterpret_cast<const P*>(x)[i] : P{};
        P pr = EPI == 0 ? reinterpret_cast<const P*>(r)[i] : P{};
        P pd = EPI == 0 ? reinterpret_cast<const P*>(dinv)[i] : P{};
        P pa = reinterpret_cast<const P*>(t1)[i];
        P pb = reinterpret_cast<const P*>(t2)[i];
#pragma unroll
        for(int k = 0; k < N; ++k)
            pk_elems<T>(px)[k] = one(pk_elems<T>(px)[k], pk_elems<T>(pr)[k], pk_elems<T>(pa)[k], pk_elems<T>(pb)[k], pk_elems<T>(pd)[k]);
        reinterpret_cast<P*>(x)[i] = px;
    }
    else if(i * N < n)
        for(int64_t e = i * N; e < n; ++e)
            x[e] = one(EPI == 1 ? x[e] : (T)0, EPI == 0 ? r[e] : (T)0, t1[e], t2[e], EPI == 0 ? dinv[e] : (T)0);
}

} // namespace ramd

using namespace ramd;

enum
{
    TNS_STORED   = 0,
    TNS_MATFREE  = 1,
    TNS_EXPLICIT = 2
};

// what form = -1 (auto) takes on an operator that qualifies for the matrix-free form: the stored one, by measurement
// (profiles/tns.md: the matrix-free passes stream both triangles of A, the stored products half of it each, and on
// constant-coefficient stencils K and K^T run the value-pattern product)
constexpr bool kTnsAutoMatrixFree = false;

struct ramd_tns_s
{
    int dtype = RAMD_F64;
    int n     = 0;
    int form  = TNS_STORED;
    int impl  = 1;
    int sym   = -1; // 1: A equals its transpose bit for bit, 0: it does not, -1: not examined (form 0, unsorted rows, explicit mode)
    // matrix-free: the operator itself (not owned) and what its arrays were at Build()
    const ramd_mat_s* A     = nullptr;
    const int*        a_rp  = nullptr;
    const int*        a_ci  = nullptr;
    const void*       a_val = nullptr;
    int*              split = nullptr;
    // stored / explicit
    ramd_mat_t K = nullptr, KT = nullptr, M = nullptr;
    ramd_vec_t dinv = nullptr, t1 = nullptr, t2 = nullptr;
    void       release()
    {
        dev_free(&split);
        ramd_mat_t* ms[] = {&K, &KT, &M};
        for(ramd_mat_t* m : ms)
        {
            if(*m)
                (void)ramd_mat_destroy(*m);
            *m = nullptr;
        }
        ramd_vec_t* vs[] = {&dinv, &t1, &t2};
        for(ramd_vec_t* v : vs)
        {
            if(*v)
                (void)ramd_vec_destroy(*v);
            *v = nullptr;
        }
    }
};

namespace
{

int tns_new_vec(int dtype, int64_t n, ramd_vec_t* out)
{
    RAMD_TRY(ramd_vec_create(dtype, out));
    return n > 0 ? ramd_vec_allocate(*out, n) : RAMD_OK;
}

// sorted rows, split positions and the comparison with the transpose; *qualifies and the reason it does not
int tns_examine(ramd_tns_s* h, const ramd_mat_s* A, bool* qualifies, std::string* why)
{
    Backend& b  = backend();
    *qualifies  = false;
    int* flags  = nullptr; // [0] unsorted, [1] differs from the transpose
    int  hf[2]  = {0, 0};
    RAMD_TRY(dev_alloc(&flags, 2));
    int s = dev_alloc(&h->split, A->nrow);
    if(s == RAMD_OK && hipMemsetAsync(flags, 0, 2 * sizeof(int), b.cur) != hipSuccess)
        s = RAMD_ERR_HIP;
    if(s == RAMD_OK)
    {
        hipLaunchKernelGGL(k_tns_split, dim3(ew_grid(A->nrow)), dim3(kBlock), 0, b.cur, A->nrow, A->rp, A->ci, h->split, flags);
        if(hipGetLastError() != hipSuccess || hipMemcpyAsync(hf, flags, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
           || hipStreamSynchronize(b.cur) != hipSuccess)
            s = RAMD_ERR_HIP;
    }
    if(s == RAMD_OK && hf[0])
        *why = "rows sorted by column (strictly ascending) are needed, and this operator's are not";
    if(s == RAMD_OK && !hf[0])
    {
        // with both sides' rows strictly ascending, A is symmetric exactly when the three arrays of A^T equal A's
        ramd_mat_t t = nullptr;
        s            = ramd_mat_create(A->dtype, &t);
        if(s == RAMD_OK)
            s = mat_transpose(A, t);
        if(s == RAMD_OK && t->nnz != A->nnz)
            hf[1] = 1;
        else if(s == RAMD_OK)
        {
            const int64_t vw = (int64_t)(val_size(A->dtype) / 4) * A->nnz;
            dev_words_differ(A->rp, t->rp, (int64_t)A->nrow + 1, flags + 1);
            dev_words_differ(A->ci, t->ci, A->nnz, flags + 1);
            dev_words_differ(A->val, t->val, vw, flags + 1);
            if(hipGetLastError() != hipSuccess
               || hipMemcpyAsync(hf + 1, flags + 1, sizeof(int), hipMemcpyDeviceToHost, b.cur) != hipSuccess
               || hipStreamSynchronize(b.cur) != hipSuccess)
                s = RAMD_ERR_HIP;
        }
        if(t)
            (void)ramd_mat_destroy(t);
        if(s == RAMD_OK)
        {
            h->sym = hf[1] ? 0 : 1;
            if(hf[1])
                *why = "a bitwise symmetric operator is needed, and this one differs from its transpose";
            else
                *qualifies = true;
        }
    }
    dev_free(&flags);
    if(s != RAMD_OK)
        RAMD_FAIL(s, "tns_build: examining the operator failed");
    return RAMD_OK;
}

// K = ExtractL(A, false) . DiagonalMatrixMultR(dinv), KT = K^T -- preconditioner_ai.cpp:548-552
int tns_build_stored(ramd_tns_s* h, ramd_mat_t A)
{
    RAMD_TRY(ramd_mat_create(h->dtype, &h->K));
    RAMD_TRY(ramd_mat_create(h->dtype, &h->KT));
    RAMD_TRY(ramd_mat_extract_tri(A, h->K, 0, 0));
    RAMD_TRY(ramd_mat_diag_mult(h->K, h->dinv, 0));
    if(h->K->nnz > 0)
        RAMD_TRY(ramd_mat_transpose(h->K, h->KT));
    else // (Transpose leaves its output alone for an empty matrix: K^T is as empty as K)
        RAMD_TRY(mat_alloc_csr(h->KT, h->n, h->n, 0));
    if(h->K->nnz <= 0)
        RAMD_HIP(hipMemsetAsync(h->KT->rp, 0, sizeof(int) * ((size_t)h->n + 1), backend().cur));
    RAMD_TRY(tns_new_vec(h->dtype, h->n, &h->t2));
    return RAMD_OK;
}

// preconditioner_ai.cpp:559-599
int tns_build_explicit(ramd_tns_s* h, ramd_mat_t A)
{
    ramd_mat_t L = nullptr, K = nullptr, KT = nullptr;
    int        s = ramd_mat_create(h->dtype, &L);
    if(s == RAMD_OK)
        s = ramd_mat_create(h->dtype, &K);
    if(s == RAMD_OK)
        s = ramd_mat_create(h->dtype, &KT);
    if(s == RAMD_OK)
        s = ramd_mat_create(h->dtype, &h->M);
    if(s == RAMD_OK)
        s = ramd_mat_extract_tri(A, L, 0, 1); // the diagonal stays in the pattern ...
    if(s == RAMD_OK)
        s = ramd_mat_scale_values(L, 0.0, 1); // ... as zeros
    if(s == RAMD_OK)
        s = ramd_mat_diag_mult(L, h->dinv, 0);
    if(s == RAMD_OK)
        s = ramd_mat_mat_mult(K, L, L);
    if(s == RAMD_OK)
        s = ramd_mat_add_scalar_values(L, -1.0, 1); // L - I
    if(s == RAMD_OK)
        s = ramd_mat_matrix_add(K, L, 1.0, -1.0, 1); // L^2 - (L - I)
    if(s == RAMD_OK)
        s = ramd_mat_transpose(K, KT);
    if(s == RAMD_OK)
        s = ramd_mat_diag_mult(KT, h->dinv, 0);
    if(s == RAMD_OK)
        s = ramd_mat_mat_mult(h->M, KT, K);
    ramd_mat_t tmp[] = {L, K, KT};
    for(ramd_mat_t m : tmp)
        if(m)
            (void)ramd_mat_destroy(m);
    return s;
}

template <typename T>
int tns_apply_t(ramd_tns_s* h, const T* r, T* x)
{
    Backend&  b    = backend();
    const T*  dinv = (const T*)h->dinv->d;
    T*        t1   = h->t1 ? (T*)h->t1->d : nullptr;
    T*        t2   = h->t2 ? (T*)h->t2->d : nullptr;
    if(h->form == TNS_EXPLICIT)
        return mat_apply_impl<T>(h->M, r, x, 0, (T)1);
    if(h->form == TNS_MATFREE)
    {
        const ramd_mat_s* A = h->A;
        if(A->rp != h->a_rp || A->ci != h->a_ci || A->val != h->a_val || A->nrow != h->n || A->format != RAMD_CSR)
            RAMD_FAIL(RAMD_ERR_STATE, "tns_apply: the operator was cleared or rebuilt after Build() (matrix-free form reads it)");
        const int    grid = (h->n + kBlock - 1) / kBlock;
        const size_t lds  = (sizeof(T) + sizeof(int)) * 4 * (size_t)kTnsCap;
#define TNS_GO(UPPER, STAGE, V, OUT)                                                                                         \
    hipLaunchKernelGGL((k_tns_tri<T, UPPER, STAGE>), dim3(grid), dim3(kBlock), lds, b.cur, h->n, A->rp, h->split, A->ci, \
                       (const T*)A->val, dinv, V, r, OUT)
        prof_begin(RAMD_PROF_PRECOND, nullptr);
        TNS_GO(false, 0, r, t1); // t1 = K r
        TNS_GO(false, 1, (const T*)t1, x); // x = (r - (t1 - K t1)) dinv
        TNS_GO(true, 0, (const T*)x, t1); // t1 = K^T x
        TNS_GO(true, 1, (const T*)t1, x); // x = x - t1 + K^T t1
#undef TNS_GO
        const hipError_t e = hipGetLastError();
        prof_end(RAMD_PROF_PRECOND, nullptr);
        RAMD_HIP(e);
        return RAMD_OK;
    }
    const int64_t np   = (h->n + Pack<T>::N - 1) / Pack<T>::N;
    const int     grid = (int)((np + kBlock - 1) / kBlock);
    RAMD_TRY(mat_apply_impl<T>(h->K, r, t1, 0, (T)1));
    RAMD_TRY(mat_apply_impl<T>(h->K, (const T*)t1, t2, 0, (T)1));
    hipLaunchKernelGGL((k_tns_epilogue<T, 0>), dim3(grid), dim3(kBlock), 0, b.cur, (int64_t)h->n, x, r, (const T*)t1, (const T*)t2,
                       dinv);
    RAMD_HIP(hipGetLastError());
    RAMD_TRY(mat_apply_impl<T>(h->KT, (const T*)x, t1, 0, (T)1));
    RAMD_TRY(mat_apply_impl<T>(h->KT, (const T*)t1, t2, 0, (T)1));
    hipLaunchKernelGGL((k_tns_epilogue<T, 1>), dim3(grid), dim3(kBlock), 0, b.cur, (int64_t)h->n, x, r, (const T*)t1, (const T*)t2,
                       dinv);
    RAMD_HIP(hipGetLastError());
    return RAMD_OK;
}

} // namespace

extern "C" {

int ramd_tns_build(ramd_mat_t mat, int impl, int form, ramd_tns_t* out)
{
    RAMD_NARROW_ONLY(mat);
    if(!mat || !out || form < -1 || form > 1)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_build: bad arguments (form is -1 auto, 0 stored, 1 matrix-free)");
    if(mat->dtype != RAMD_F64 && mat->dtype != RAMD_F32)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_build: a real operator expected");
    if(mat->nrow != mat->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_build: the operator is not square");
    if(mat->nrow <= 0 || (mat->format == RAMD_CSR && mat->nnz <= 0))
        RAMD_FAIL(RAMD_ERR_ARG, "tns_build: the operator is empty");
    if(form == 1 && !impl)
        RAMD_FAIL(RAMD_ERR_REFUSED, "tns_build: the matrix-free form exists for the implicit mode only (Set(true))");
    if(form == 1 && mat->format != RAMD_CSR)
        RAMD_FAIL(RAMD_ERR_REFUSED, "tns_build: the matrix-free form refused: an operator in CSR format is needed");
    ramd_tns_s* h = new ramd_tns_s;
    h->dtype      = mat->dtype;
    h->n          = mat->nrow;
    h->impl       = impl ? 1 : 0;
    // ELL / HYB / COO operators: the primitives work on a CSR copy
    ramd_mat_t csr = nullptr;
    int        s   = RAMD_OK;
    if(mat->format != RAMD_CSR)
    {
        s = ramd_mat_clone(mat, &csr);
        if(s == RAMD_OK)
            s = ramd_mat_convert(csr, RAMD_CSR);
    }
    ramd_mat_t A = csr ? csr : mat;
    if(s == RAMD_OK)
        s = ramd_vec_create(h->dtype, &h->dinv);
    if(s == RAMD_OK)
        s = ramd_mat_extract_inv_diag(A, h->dinv);
    bool        qualifies = false;
    std::string why;
    // (form 0 takes the stored form whatever A is: no transpose of A, no comparison, the symmetry stays unexamined)
    if(s == RAMD_OK && impl && !csr && form != 0)
        s = tns_examine(h, A, &qualifies, &why);
    if(s == RAMD_OK && form == 1 && !qualifies)
    {
        h->release();
        delete h;
        RAMD_FAIL(RAMD_ERR_REFUSED, "tns_build: the matrix-free form refused: " + why);
    }
    if(s == RAMD_OK)
    {
        if(!impl)
            h->form = TNS_EXPLICIT;
        else if(form == 1 || (form == -1 && qualifies && kTnsAutoMatrixFree))
            h->form = TNS_MATFREE;
        else
            h->form = TNS_STORED;
    }
    if(s == RAMD_OK && h->form != TNS_EXPLICIT)
        s = tns_new_vec(h->dtype, h->n, &h->t1);
    if(s == RAMD_OK && h->form == TNS_MATFREE)
    {
        h->A     = mat;
        h->a_rp  = mat->rp;
        h->a_ci  = mat->ci;
        h->a_val = mat->val;
    }
    else if(s == RAMD_OK)
    {
        dev_free(&h->split);
        s = h->form == TNS_STORED ? tns_build_stored(h, A) : tns_build_explicit(h, A);
    }
    if(csr)
        (void)ramd_mat_destroy(csr);
    if(s != RAMD_OK)
    {
        h->release();
        delete h;
        return s;
    }
    *out = h;
    return RAMD_OK;
}

int ramd_tns_convert(ramd_tns_t h, int format)
{
    if(!h)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_convert: null plan");
    if(h->form == TNS_MATFREE)
        RAMD_FAIL(RAMD_ERR_STATE, "tns_convert: the matrix-free form stores no matrix (build the stored form, form = 0)");
    ramd_mat_t ms[] = {h->M, h->K, h->KT};
    for(ramd_mat_t m : ms)
    {
        if(!m || m->format == format || m->nnz <= 0)
            continue;
        if(m->format != RAMD_CSR && format != RAMD_CSR)
            RAMD_TRY(ramd_mat_convert(m, RAMD_CSR));
        const int s = ramd_mat_convert(m, format);
        if(s != RAMD_OK && s != RAMD_ERR_REFUSED) // (a refused ELL conversion leaves the matrix in CSR, as ConvertTo does)
            return s;
    }
    return RAMD_OK;
}

int ramd_tns_apply(ramd_tns_t h, ramd_vec_t rhs, ramd_vec_t x)
{
    if(!h || !rhs || !x || rhs == x)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_apply: bad arguments (rhs and x must be two vectors)");
    if(rhs->dtype != h->dtype || x->dtype != h->dtype || rhs->n != h->n || x->n != h->n)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_apply: vector size / type mismatch");
    if(h->dtype == RAMD_F64)
        return tns_apply_t<double>(h, (const double*)rhs->d, (double*)x->d);
    return tns_apply_t<float>(h, (const float*)rhs->d, (float*)x->d);
}

int ramd_tns_info(ramd_tns_t h, int64_t* out8)
{
    if(!h || !out8)
        RAMD_FAIL(RAMD_ERR_ARG, "tns_info: bad arguments");
    const ramd_mat_s* m = h->form == TNS_EXPLICIT ? h->M : h->K;
    out8[0]             = h->form;
    out8[1]             = h->impl;
    out8[2]             = h->sym;
    out8[3]             = h->n;
    out8[4]             = m ? m->nnz : 0;
    out8[5]             = m ? m->format : 0;
    out8[6]             = h->KT ? h->KT->format : 0;
    out8[7]             = 0;
    return RAMD_OK;
}

int ramd_tns_destroy(ramd_tns_t h)
{
    if(h)
    {
        h->release();
        delete h;
    }
    return RAMD_OK;
}

} // extern "C"
