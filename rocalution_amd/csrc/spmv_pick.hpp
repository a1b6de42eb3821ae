// spmv_pick.hpp -- which kernel a CSR / ELL product takes: the switches of the process, the facts of a matrix, and one pure
// function from both to a kernel (or to the analysis that has to run first).  Host only: no HIP header, nothing of ramd_mat_s;
// spmv.hip fills the facts (facts_of), runs the analyses (spmv_prepare) and launches (launch_csr), tests/drivers/spmv_pick_driver.cpp calls
// the same functions from a plain C++ program.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace ramd
{

// (the kernels' constants, restated: spmv.hip and matrix_impl.hpp assert that they agree)
constexpr int kPickRows    = 256; // kCsrRows
constexpr int kPickChunk   = 2048; // kCsrChunk
constexpr int kPickPatMax  = 64; // kPatMax
constexpr int kPickPatMaxW = 28; // kPatMaxW

// Every RAMD_CSR_* switch, RAMD_ELL2 and RAMD_CG_LATDIR: read from the environment once per process (spmv_switches), here and
// nowhere else.  All of them are A/B switches of bit-identical kernels.
struct SpmvSwitches
{
    // structured operators: columns from a row-pattern dictionary (csr_analyse_pattern); analysed once, on the first product
    // of a matrix with >= 2^20 entries (1: every matrix, 0: never).  ELL / HYB and the multi-colour sweeps follow it too
    int pat = -1;
    // ... whose values are a function of the pattern as well (k_csr_patv) -- unset: matrices that have row patterns are tried;
    // 0: never; 1: also analyse the patterns of every matrix whatever its size (as pat = 1)
    int patv = -1;
    // rows beyond k_csr_pat2's reach (more than 7 entries: the 27-point operator) take k_csr_patv too -- CG + Jacobi on the
    // 27-point operator at 256^3: 0.50 against 1.27 ms per iteration with k_csr_wr, three alternating runs per side
    // (profiles/valpat_headline.txt).  0: they keep their kernels (A/B)
    int patv_long = 1;
    // the lattice form of the value-pattern product (k_csr_lat) -- 0: off; 1: lattice operators of 2^16 rows and more; 2: any size
    int lat = 1;
    // CG + Jacobi on a lattice operator, direction update and product in one launch (k_cg_lat).  0: the loop keeps its three
    // launches (A/B runs)
    int cg_latdir = 1;
    // long rows (mean > 16 entries): four lanes per row (k_csr_q4) -- 0 / 1: force, A/B experiments.  Measured EQUAL to
    // k_csr_tr on the shell surrogate (0.162 vs 0.160 ms): opt-in
    int q4 = -1;
    // x tiles of a structured product in LDS, opt-in (1: k_csr_xl; default: the gather form k_csr_tr<PAT>)
    int xl = 0;
    // rows sharing the column list of their predecessor (FE matrices), opt-in.  Measured on the af_shell10-class matrix
    // (profiles/r03_spmv_shell_variants.txt): 9.4 instead of 12.6 bytes per entry moved, and 0.235 ms instead of 0.159 ms -- the
    // product is bound by the dependent gather rounds of the row walk (five per 35-entry row, one row in four lanes active per
    // 2048-entry pass), not by bytes; the per-entry choice between the leader's staged columns and the row's own costs more
    // than the column packets saved.  Kept under the same bit-exact tests as an experiment.
    int grp = 0;
    // two row blocks per workgroup with their memory phases overlapped (k_csr_pat2), where a row block fits one LDS pass
    // (0: k_csr_tr<PAT>; A/B experiments)
    int pat2 = 1;
    // k_csr_pat2 without row offsets (measured without gain, 1.80-1.85 vs 1.73-1.92 ms plain and 2.03-2.10 vs 2.02-2.04 ms with
    // the dot in alternating runs: 5 % fewer bytes do nothing for a product bound by its latency chain, the scan adds two
    // barriers -- opt-in)
    int norp = 0;
    // 1: the compact block offsets for the general kernel too -- measured without effect there, 2.36-2.52 vs 2.45-2.52 ms with
    // the columns read at 512^3 and 0.157 vs 0.157 ms on the shell surrogate: that kernel runs at the stream rate of its bytes
    // already
    int blkrp = 0;
    // k_csr_pat2's structure with the columns read, for matrices of short rows (every row block fits one LDS pass) -- measured
    // SLOWER than k_csr_tr, 2.52-2.55 vs 2.38-2.40 ms at 512^3 in alternating runs: with the columns read the product runs at the
    // stream rate of its 14.2 GB and the extra registers only cost occupancy -- opt-in: 1; 2: also small matrices, for the tests
    int col2 = 0;
    // the next pass requested before the row walk (measured SLOWER on the config-3 surrogate: 0.173 against 0.154-0.159 ms in
    // alternating runs -- opt-in)
    int pipe = 0;
    // wave-private passes -- 0 / 1: force; default: rows of 16+ entries, unless they are the rows of a stencil (csr_analyse_shift)
    int w4       = -1;
    int w4_waves = 4; // (1: one wave per workgroup)
    int wp       = 1; // (0: k_csr_w4 where k_csr_wp would run)
    // rows of 16+ entries that walk their rows in k_csr_tr (stencils; row patterns of long rows): entries per LDS pass -- 2048 /
    // 4096 / 8192; 4096 measured best on the 27-point operator: 1.13 ms against 1.66 ms at 8192 with row patterns
    int lchunk = -1;
    // ... and those that would take its 4096-entry passes: the wave-private row walk (k_csr_wr) (0: k_csr_tr in long chunks)
    int wr    = 1;
    int wr_gw = 14; // (gathers in flight per row: 8 / 14 / 28)
    // ELL / HYB: two rows per thread (k_ell2) where the pairs are aligned -- 0 / 1: force; default: 2^16 rows and more.  With
    // patterns eight slots per batch: 126 registers, 1.81-1.88 against 2.12-2.19 ms at 512^3; eight slots per batch with the
    // columns read need 206 registers -- 2 waves per SIMD -- and ran at 3.8-4.0 ms against k_ell's 2.4 ms, so with the columns
    // read four slots per batch (76 registers, 6 waves per SIMD): 2.27-2.48 ms against k_ell's 2.42-2.55 ms in alternating
    // runs, a few per cent, taken
    int ell2 = -1;
};

// the switches as `get` (getenv, or a test's table) gives them; unset: the defaults above
template <typename Get>
inline SpmvSwitches spmv_switches_read(Get get)
{
    SpmvSwitches s;
    const struct
    {
        const char* name;
        int*        v;
    } all[] = {{"RAMD_CSR_PAT", &s.pat},           {"RAMD_CSR_PATV", &s.patv},     {"RAMD_CSR_PATV_LONG", &s.patv_long},
               {"RAMD_CSR_LAT", &s.lat},           {"RAMD_CG_LATDIR", &s.cg_latdir}, {"RAMD_CSR_Q4", &s.q4},
               {"RAMD_CSR_XL", &s.xl},             {"RAMD_CSR_GRP", &s.grp},       {"RAMD_CSR_PAT2", &s.pat2},
               {"RAMD_CSR_NORP", &s.norp},         {"RAMD_CSR_BLKRP", &s.blkrp},   {"RAMD_CSR_COL2", &s.col2},
               {"RAMD_CSR_PIPE", &s.pipe},         {"RAMD_CSR_W4", &s.w4},         {"RAMD_CSR_W4_WAVES", &s.w4_waves},
               {"RAMD_CSR_WP", &s.wp},             {"RAMD_CSR_LCHUNK", &s.lchunk}, {"RAMD_CSR_WR", &s.wr},
               {"RAMD_CSR_WR_GW", &s.wr_gw},       {"RAMD_ELL2", &s.ell2}};
    for(const auto& e : all)
        if(const char* t = get(e.name))
            *e.v = std::atoi(t);
    return s;
}
inline const SpmvSwitches& spmv_switches()
{
    static const SpmvSwitches s = spmv_switches_read([](const char* name) { return (const char*)std::getenv(name); });
    return s;
}

// what the decision looks at in a matrix (ramd_mat_s; an ELL block: nnz = nrow * ell_width, its slots)
struct CsrFacts
{
    int     nrow = 0, ncol = 0;
    int64_t nnz  = 0;
    bool    wide = false; // 64-bit row offsets
    int     pat_state = 0; // 0 not analysed, 1 dictionary, -1 none
    bool    pat_off   = false; // ramd_mat_pattern_use(m, 0)
    int     pat_n = 0, pat_maxlen = 0; // dictionary entries, the longest of them
    int     pat_vstate = 0; // values: 0 not analysed, 1 from the dictionary, -1 not a function of the pattern
    bool    pat_vdict  = false; // ... and the value dictionary exists
    int     lat_state = 0, xl_state = 0, grp_state = 0; // 0 not analysed, 1 in use, -1 not such a matrix
    int     blk_span   = 0; // 0 not measured, -1 empty, else the most entries a row block stages
    int     shift_rows = -1; // -1 not analysed, 0 / 1
};

// the analyses a choice may wait for: csr_analyse_pattern (ell_analyse_pattern), _values, _lattice, _xl, _groups, the block
// offsets with the longest span among them, csr_analyse_shift
enum SpmvNeed { NEED_NONE = 0, NEED_PATTERNS, NEED_VALUES, NEED_LATTICE, NEED_XL, NEED_GROUPS, NEED_SPAN, NEED_SHIFT };
// the kernels: k_csr_lat, k_csr_patv, k_csr_q4, k_csr_xl, k_csr_pat2<PAT>, <PAT, NORP> and with the columns read, k_csr_wr<pat, gw>,
// k_csr_tr<PAT, chunk>, <GRP>, k_csr_wp, k_csr_w4<waves>, k_csr_tr<chunk>, <PIPE>, k_csr_wide<pat>, k_ell<pat>, k_ell2<pat>
enum SpmvKernel { K_NONE = 0, K_LAT, K_PATV, K_Q4, K_XL, K_PAT2, K_PAT2_NORP, K_COL2, K_WR, K_TR_PAT, K_TR_GRP, K_WP, K_W4, K_TR,
                  K_TR_PIPE, K_WIDE, K_ELL, K_ELL2 };
struct CsrPick
{
    SpmvNeed   need   = NEED_NONE; // != NEED_NONE: run this analysis and ask again; the rest is not set
    SpmvKernel kernel = K_NONE;
    bool       pat    = false; // the kernel takes its columns from the dictionary
    bool       blk_rp = false; // derived arrays the launch builds first, where the matrix has none yet: blk_rp ...
    int        chunk  = 0; // K_TR_PAT, K_TR: entries per LDS pass; K_W4: waves per workgroup
    int        gw     = 0; // K_WR: gathers in flight per row
    bool       wav_rp = false; // ... and wav_rp
    CsrPick() = default;
    CsrPick(SpmvNeed n) : need(n) {}
    CsrPick(SpmvKernel k, bool p, bool b, int c = 0, int g = 0, bool w = false) : kernel(k), pat(p), blk_rp(b), chunk(c), gw(g), wav_rp(w) {}
};

// The product of a CSR matrix (mode 0: y = A x, 1: y += s A x, 2: Jacobi sweep; dot: fused <x, y>), kernels in priority order.
// A matrix either uses its dictionary (everything down to K_TR_PAT) or reads its columns (everything after); one with 64-bit
// row offsets has the value-pattern kernels, which read no row offsets, and k_csr_wide.
inline CsrPick csr_pick(const CsrFacts& f, const SpmvSwitches& sw, int mode, bool dot)
{
    (void)dot; // (every kernel has its fused-dot form)
    if(f.pat_state == 0 && sw.pat != 0 && (sw.pat > 0 || sw.patv > 0 || f.nnz >= (1 << 20)))
        return NEED_PATTERNS;
    const bool    rows16 = f.nnz >= (int64_t)16 * f.nrow; // rows of 16+ entries
    const int     gw     = sw.wr_gw == 8 ? 8 : (sw.wr_gw == 14 ? 14 : 28);
    const bool    big    = f.nrow >= (1 << 16);
    if(sw.pat != 0 && f.pat_state == 1 && !f.pat_off)
    {
        const bool one_pass = kPickRows * f.pat_maxlen + 3 <= kPickChunk; // a row block fits one LDS pass
        // values from the dictionary too -- unless a switch asks for a columns-only kernel by name: xl (the opt-in experiment
        // keeps its kernel), pat2 = 0 (k_csr_tr<PAT>), norp = 1 (k_csr_pat2<NORP>)
        if(sw.patv != 0 && sw.xl == 0 && sw.pat2 != 0 && sw.norp == 0 && f.pat_n > 0 && f.pat_n <= kPickPatMax && f.pat_maxlen > 0
           && f.pat_maxlen <= kPickPatMaxW && (one_pass || sw.patv_long != 0))
        {
            if(f.pat_vstate == 0)
                return NEED_VALUES;
            // the plain product and the product with a fused dot of a lattice operator: tiles of x in LDS marched along z
            const bool try_lat = mode == 0 && sw.lat != 0 && (sw.lat >= 2 || big);
            if(try_lat && f.lat_state == 0)
                return NEED_LATTICE; // (without a value dictionary the analysis says at once: not such a matrix)
            if(f.pat_vstate == 1 && f.pat_vdict)
                return CsrPick(try_lat && f.lat_state == 1 ? K_LAT : K_PATV, true, false);
        }
        if(f.wide)
            return CsrPick(K_WIDE, true, false);
        if(sw.xl != 0 && f.xl_state == 0)
            return NEED_XL;
        const bool blk_rp = sw.blkrp != 0 && big;
        if(sw.xl != 0 && f.xl_state == 1)
            return CsrPick(K_XL, true, true);
        if(sw.pat2 != 0 && f.pat_maxlen > 0 && one_pass)
            return CsrPick(sw.norp != 0 ? K_PAT2_NORP : K_PAT2, true, true);
        const int chunk = !(rows16 && !(sw.q4 > 0)) ? 0 : (sw.lchunk >= 0 ? sw.lchunk : 4096);
        if(sw.wr != 0 && chunk >= 4096 && sw.pipe == 0)
            return CsrPick(K_WR, true, blk_rp, 0, gw, true);
        return CsrPick(K_TR_PAT, true, blk_rp, chunk == 8192 || chunk == 4096 ? chunk : kPickChunk);
    }
    if(f.wide)
        return CsrPick(K_WIDE, false, false);
    if(sw.grp > 0 && f.grp_state == 0 && f.pat_state != 1)
        return NEED_GROUPS;
    if(sw.q4 > 0)
        return CsrPick(K_Q4, false, false);
    bool blk_rp = sw.blkrp != 0 && big;
    if(sw.grp != 0 && f.grp_state == 1 && !f.pat_off)
        return CsrPick(K_TR_GRP, false, blk_rp);
    if(sw.col2 != 0 && (big || sw.col2 == 2) && f.nnz <= (int64_t)8 * f.nrow && f.blk_span >= 0)
    {
        if(f.blk_span == 0)
            return NEED_SPAN;
        blk_rp = true;
        if(f.blk_span <= kPickChunk)
            return CsrPick(K_COL2, false, true);
    }
    if(rows16 && sw.w4 < 0 && f.shift_rows < 0)
        return NEED_SHIFT;
    if(sw.w4 >= 0 ? sw.w4 != 0 : (rows16 && f.shift_rows != 1))
    {
        if(sw.wp != 0 && sw.w4_waves != 1)
            return CsrPick(K_WP, false, blk_rp);
        return CsrPick(K_W4, false, blk_rp, sw.w4_waves == 1 ? 1 : 4);
    }
    const int chunk = !rows16 ? 0 : (sw.lchunk >= 0 ? sw.lchunk : 4096);
    if(sw.wr != 0 && chunk >= 4096 && sw.pipe == 0)
        return CsrPick(K_WR, false, blk_rp, 0, gw, true);
    if(chunk >= 4096)
        return CsrPick(K_TR, false, blk_rp, 4096);
    return CsrPick(sw.pipe != 0 ? K_TR_PIPE : K_TR, false, blk_rp, kPickChunk);
}

// CG + Jacobi with direction update and product in one launch (k_cg_lat): where the plain product is the lattice kernel's.
// (Narrower in form than the rule it replaces, which did not restate k_csr_patv's bound on the pattern length -- not in effect:
//  lat_state becomes 1 only behind that bound, and the switches do not change while a process runs.)
inline bool cg_lat_pick(const CsrFacts& f, const SpmvSwitches& sw)
{
    return sw.cg_latdir != 0 && !f.wide && f.nnz > 0 && f.nrow == f.ncol && csr_pick(f, sw, 0, false).kernel == K_LAT;
}

// ... and of the ELL block of an ELL / HYB matrix (f.nnz: its slots)
inline CsrPick ell_pick(const CsrFacts& f, const SpmvSwitches& sw)
{
    if(f.pat_state == 0 && sw.pat != 0 && (sw.pat > 0 || f.nnz >= (1 << 20)))
        return NEED_PATTERNS;
    // two rows per thread where the pairs are aligned: an even number of rows
    const bool two = f.nrow % 2 == 0 && f.nrow > 0 && (sw.ell2 >= 0 ? sw.ell2 != 0 : f.nrow >= (1 << 16));
    return CsrPick(two ? K_ELL2 : K_ELL, sw.pat != 0 && f.pat_state == 1 && !f.pat_off, false);
}

} // namespace ramd
