// host_analysis.hip -- setup steps that the reference itself runs SERIALLY ON THE HOST in both of
// its backends.  MultiColoring: the reference HIP backend copies row_offset/col to the host and runs
// the same greedy loop as the host backend (src/base/hip/hip_matrix_csr.cpp:3915-4060 ==
// src/base/host/host_matrix_csr.cpp:2469-2599).  The colour ORDER decides the permutation and with it
// every MC-SGS result, so this stays a sequential first-fit sweep with identical tie-breaking:
//   natural row order; neighbours = row entries AND column (CSC) entries; colours numbered from 1;
//   perm[i] = offset[colour(i)]++  (stable inside a colour).
#include "common.hpp"
#include "matrix_impl.hpp"

#include <vector>

using namespace ramd;

extern "C" int ramd_mat_multicoloring(ramd_mat_t m, int* num_colors, int* size_colors, ramd_vec_t perm)
{
    RAMD_NARROW_ONLY(m);
    if(!m || !num_colors || !size_colors || !perm)
        RAMD_FAIL(RAMD_ERR_ARG, "MultiColoring: null argument");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(perm->dtype != RAMD_I32)
        RAMD_FAIL(RAMD_ERR_ARG, "MultiColoring: permutation must be an int32 vector");
    if(m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "MultiColoring: square matrix expected");
    // device sweep when it applies (structurally symmetric pattern, <= 64 colours): same colours;
    // RAMD_COLORING=host forces the serial sweep below
    static const bool force_host = [] {
        const char* e = getenv("RAMD_COLORING");
        return e && std::string(e) == "host";
    }();
    if(!force_host)
    {
        int s = multicoloring_device(m, num_colors, size_colors, perm);
        if(s != RAMD_ERR_UNSUPPORTED)
            return s;
    }
    Backend&  b   = backend();
    const int n   = m->nrow;
    const int64_t nnz = m->nnz;
    std::vector<int> rp((size_t)n + 1), ci((size_t)nnz);
    RAMD_HIP(hipMemcpyAsync(rp.data(), m->rp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, b.cur));
    if(nnz > 0)
        RAMD_HIP(hipMemcpyAsync(ci.data(), m->ci, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));

    // column view (who has an entry in my column)
    std::vector<int> csc_ptr((size_t)n + 1, 0), csc_ind((size_t)nnz);
    for(int64_t i = 0; i < nnz; ++i)
        csc_ptr[ci[i] + 1] += 1;
    for(int i = 1; i <= n; ++i)
        csc_ptr[i] += csc_ptr[i - 1];
    {
        std::vector<int> cur(csc_ptr.begin(), csc_ptr.end() - 1);
        for(int i = 0; i < n; ++i)
            for(int k = rp[i]; k < rp[i + 1]; ++k)
                csc_ind[cur[ci[k]]++] = i;
    }

    std::vector<int>  color((size_t)n, 0);
    std::vector<char> used;
    int               ncol = 0;
    for(int ai = 0; ai < n; ++ai)
    {
        color[ai] = 1;
        used.assign((size_t)ncol + 2, 0);
        for(int aj = rp[ai]; aj < rp[ai + 1]; ++aj)
            if(ai != ci[aj])
                used[color[ci[aj]]] = 1;
        for(int aj = csc_ptr[ai]; aj < csc_ptr[ai + 1]; ++aj)
            if(ai != csc_ind[aj])
                used[color[csc_ind[aj]]] = 1;
        const int count = rp[ai + 1] - rp[ai] + csc_ptr[ai + 1] - csc_ptr[ai];
        for(int aj = 0; aj < count; ++aj)
        {
            if(used[color[ai]])
                ++color[ai];
            else
                break;
        }
        if(color[ai] > ncol)
            ncol = color[ai];
    }
    std::vector<int> offsets((size_t)std::max(ncol, 1), 0);
    for(int i = 0; i < ncol; ++i)
        size_colors[i] = 0;
    for(int i = 0; i < n; ++i)
        ++size_colors[color[i] - 1];
    int total = 0;
    for(int i = 1; i < ncol; ++i)
    {
        total += size_colors[i - 1];
        offsets[i] = total;
    }
    std::vector<int> hperm((size_t)n);
    for(int i = 0; i < n; ++i)
        hperm[i] = offsets[color[i] - 1]++;
    *num_colors = ncol;
    RAMD_TRY(ramd_vec_allocate(perm, n));
    if(n > 0)
        RAMD_TRY(ramd_vec_copy_from_host(perm, hperm.data()));
    return RAMD_OK;
}

// RSCoarsening, the Greedy strategy of RugeStuebenAMG (host_matrix_csr.cpp:6782-7058): the classical first pass.  The
// sweep always takes the undecided point with the largest measure lambda (number of points it strongly influences,
// fine ones counted twice) and the order among equal measures decides the C/F map, so it is sequential; the reference's
// HIP backend does not provide it either and runs the host loop.  Pattern and values go to the host, cfmap (1 coarse,
// 2 fine) and S (per entry: 1 where the row strongly depends on the column) come back.  The priority lists are the
// reference's: one array of points grouped by measure, ptr[m] the start of group m and cnt[m] its size; a point whose
// measure rises swaps with the last of its group, one whose measure falls with the first; the sweep takes the array
// from the back.
template <typename T>
static int rs_greedy_t(const ramd_mat_s* m, float eps, ramd_vec_s* vcf, ramd_vec_s* vS)
{
    Backend&      b   = backend();
    const int     n   = m->nrow;
    const int64_t nnz = m->nnz;
    std::vector<int> rp((size_t)n + 1), ci((size_t)nnz);
    std::vector<T>   va((size_t)nnz);
    RAMD_HIP(hipMemcpyAsync(rp.data(), m->rp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipMemcpyAsync(ci.data(), m->ci, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipMemcpyAsync(va.data(), m->val, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost, b.cur));
    RAMD_HIP(hipStreamSynchronize(b.cur));

    std::vector<int> cf((size_t)n, 0), S((size_t)nnz, 0);
    for(int i = 0; i < n; ++i)
    {
        T    lo = (T)0, hi = (T)0;
        bool neg_diag = false;
        for(int j = rp[i]; j < rp[i + 1]; ++j)
        {
            const T v = va[j];
            if(ci[j] == i)
                neg_diag = v < (T)0;
            else
            {
                lo = (lo < v) ? lo : v;
                hi = (hi > v) ? hi : v;
            }
        }
        const T cond = (neg_diag ? hi : lo) * (T)eps;
        for(int j = rp[i]; j < rp[i + 1]; ++j)
            S[j] = (ci[j] != i && va[j] < cond) ? 1 : 0;
        if(cond == (T)0) // no strong dependence at all: the point stays fine
            cf[i] = 2;
    }
    // S transposed: who depends strongly on me
    std::vector<int> tp((size_t)n + 1, 0), ti;
    for(int64_t j = 0; j < nnz; ++j)
        if(S[j])
            ++tp[ci[j] + 1];
    for(int i = 0; i < n; ++i)
        tp[i + 1] += tp[i];
    ti.resize((size_t)tp[n]);
    {
        std::vector<int> cur(tp.begin(), tp.end() - 1);
        for(int i = 0; i < n; ++i)
            for(int j = rp[i]; j < rp[i + 1]; ++j)
                if(S[j])
                    ti[cur[ci[j]]++] = i;
    }
    std::vector<int> lambda((size_t)n), ptr((size_t)n + 1, 0), cnt((size_t)n, 0), at((size_t)n), pos((size_t)n);
    for(int i = 0; i < n; ++i)
    {
        int w = 0;
        for(int j = tp[i]; j < tp[i + 1]; ++j)
            w += (cf[ti[j]] == 0) ? 1 : 2;
        lambda[i] = w; // (a measure never exceeds 2 (n - 1) in theory; the lists below hold n groups, as the reference's)
        if(w + 1 > n)
            RAMD_FAIL(RAMD_ERR_UNSUPPORTED, "RSCoarsening: a point's measure exceeds the number of rows");
        ++ptr[w + 1];
    }
    for(int i = 1; i <= n; ++i)
        ptr[i] += ptr[i - 1];
    for(int i = 0; i < n; ++i)
    {
        const int w = lambda[i], q = ptr[w] + cnt[w]++;
        at[q]  = i;
        pos[i] = q;
    }
    auto swap_to = [&](int point, int q) {
        const int o = pos[point], other = at[q];
        pos[point] = q;
        pos[other] = o;
        at[o]      = other;
        at[q]      = point;
    };
    for(int top = n - 1; top >= 0; --top)
    {
        const int i = at[top], w = lambda[i];
        if(w == 0)
        {
            for(int a = 0; a < n; ++a)
                if(cf[a] == 0)
                    cf[a] = 1;
            break;
        }
        --cnt[w];
        if(cf[i] == 2)
            continue;
        cf[i] = 1;
        for(int j = tp[i]; j < tp[i + 1]; ++j)
        {
            const int c = ti[j];
            if(cf[c] != 0)
                continue;
            cf[c] = 2;
            for(int jj = rp[c]; jj < rp[c + 1]; ++jj)
            {
                if(!S[jj])
                    continue;
                const int cc = ci[jj], wc = lambda[cc];
                if(cf[cc] != 0 || wc >= n - 1)
                    continue;
                swap_to(cc, ptr[wc] + cnt[wc] - 1);
                --cnt[wc];
                ++cnt[wc + 1];
                ptr[wc + 1] = ptr[wc] + cnt[wc];
                ++lambda[cc];
            }
        }
        for(int j = rp[i]; j < rp[i + 1]; ++j)
        {
            if(!S[j])
                continue;
            const int c = ci[j], wc = lambda[c];
            if(cf[c] != 0 || wc == 0)
                continue;
            swap_to(c, ptr[wc]);
            --cnt[wc];
            ++cnt[wc - 1];
            ++ptr[wc];
            --lambda[c];
        }
    }
    RAMD_TRY(ramd_vec_allocate(vcf, n));
    RAMD_TRY(ramd_vec_allocate(vS, nnz));
    if(n > 0)
        RAMD_TRY(ramd_vec_copy_from_host(vcf, cf.data()));
    if(nnz > 0)
        RAMD_TRY(ramd_vec_copy_from_host(vS, S.data()));
    return RAMD_OK;
}

extern "C" int ramd_mat_rs_coarsening(ramd_mat_t m, float eps, ramd_vec_t cfmap, ramd_vec_t S)
{
    RAMD_NARROW_ONLY(m);
    if(!m || !cfmap || !S)
        RAMD_FAIL(RAMD_ERR_ARG, "null handle");
    if(m->format != RAMD_CSR)
        return RAMD_ERR_UNSUPPORTED;
    if(cfmap->dtype != RAMD_I32 || S->dtype != RAMD_I32 || m->nrow != m->ncol)
        RAMD_FAIL(RAMD_ERR_ARG, "RSCoarsening: square matrix and int vectors expected");
    if(m->nnz <= 0)
        return RAMD_OK;
    return (m->dtype == RAMD_F64) ? rs_greedy_t<double>(m, eps, cfmap, S) : rs_greedy_t<float>(m, eps, cfmap, S);
}
