"""Which kernel a CSR / ELL product takes: a restatement of launch_csr / launch_csr_patv / launch_csr_wide / launch_ell as they
stood before csrc/spmv_pick.hpp existed -- boolean by boolean and in their order, static by static, so that it can be held beside
that code.  Deliberately NOT written from the header: tests/test_cpu_spmv_pick.py compares the header with this file.

Where the old code ran a lazy analysis (`if(state == 0 ...) analyse`), this returns ("need", name) instead; asked again with
the state moved off 0 it goes on from there, as the old function did in one body."""

ROWS, CHUNK, PAT_MAX, PAT_MAXW = 256, 2048, 64, 28  # kCsrRows, kCsrChunk, kPatMax, kPatMaxW

# the function-local statics of the old code: name -> value where the variable is unset
DEFAULTS = {"RAMD_CSR_PAT": -1, "RAMD_CSR_PATV": -1, "RAMD_CSR_PATV_LONG": 1, "RAMD_CSR_LAT": 1, "RAMD_CG_LATDIR": 1, "RAMD_CSR_Q4": -1,
            "RAMD_CSR_XL": 0, "RAMD_CSR_GRP": 0, "RAMD_CSR_PAT2": 1, "RAMD_CSR_NORP": 0, "RAMD_CSR_BLKRP": 0, "RAMD_CSR_COL2": 0,
            "RAMD_CSR_PIPE": 0, "RAMD_CSR_W4": -1, "RAMD_CSR_W4_WAVES": 4, "RAMD_CSR_WP": 1, "RAMD_CSR_LCHUNK": -1, "RAMD_CSR_WR": 1,
            "RAMD_CSR_WR_GW": 14, "RAMD_ELL2": -1}
# kernel numbers: SpmvKernel of csrc/spmv_pick.hpp, in the order the issue lists them
(K_NONE, K_LAT, K_PATV, K_Q4, K_XL, K_PAT2, K_PAT2_NORP, K_COL2, K_WR, K_TR_PAT, K_TR_GRP, K_WP, K_W4, K_TR, K_TR_PIPE, K_WIDE,
 K_ELL, K_ELL2) = range(18)
FACTS = ("nrow", "ncol", "nnz", "wide", "pat_state", "pat_off", "pat_n", "pat_maxlen", "pat_vstate", "pat_vdict", "lat_state",
         "xl_state", "grp_state", "blk_span", "shift_rows")


def switches(env):
    """env: {name: str or int} of the variables that are set"""
    return {k: (int(env[k]) if k in env else d) for k, d in DEFAULTS.items()}


def kernel(k, pat=False, chunk=0, gw=0, blk_rp=False, wav_rp=False):
    return ("kernel", k, chunk, gw, int(bool(pat)), int(bool(blk_rp)), int(bool(wav_rp)))


def _patv(f, sw, mode):
    """launch_csr_patv: None where *taken stays false"""
    patv_switches = (sw["RAMD_CSR_PATV"] != 0 and sw["RAMD_CSR_PAT"] != 0 and sw["RAMD_CSR_XL"] == 0 and sw["RAMD_CSR_PAT2"] != 0
                     and sw["RAMD_CSR_NORP"] == 0)
    if not patv_switches or f["pat_state"] != 1 or f["pat_off"] or f["pat_n"] <= 0 or f["pat_n"] > PAT_MAX:
        return None
    maxlen = f["pat_maxlen"]
    if maxlen <= 0 or maxlen > PAT_MAXW or (ROWS * maxlen + 3 > CHUNK and sw["RAMD_CSR_PATV_LONG"] == 0):
        return None
    if f["pat_vstate"] == 0:
        return ("need", "values")
    lat_admits = sw["RAMD_CSR_LAT"] != 0 and (sw["RAMD_CSR_LAT"] >= 2 or f["nrow"] >= (1 << 16))
    try_lat = mode == 0 and lat_admits
    if f["pat_vstate"] != 1 or not f["pat_vdict"]:
        if try_lat and f["lat_state"] == 0:
            return ("need", "lattice")  # (the old code set lat_state = -1 here itself; csr_analyse_lattice does the same at once)
        return None
    if try_lat:
        if f["lat_state"] == 0:
            return ("need", "lattice")
        if f["lat_state"] == 1:
            return kernel(K_LAT, pat=True)
    return kernel(K_PATV, pat=True)


def csr_pick(f, sw, mode, dot):
    """launch_csr (f["wide"]: launch_csr_wide)"""
    pat_env, q4_env = sw["RAMD_CSR_PAT"], sw["RAMD_CSR_Q4"]
    if f["pat_state"] == 0 and pat_env != 0 and (pat_env > 0 or sw["RAMD_CSR_PATV"] > 0 or f["nnz"] >= (1 << 20)):
        return ("need", "patterns")
    use_pat = pat_env != 0 and f["pat_state"] == 1 and not f["pat_off"]
    if use_pat:
        taken = _patv(f, sw, mode)
        if taken is not None:
            return taken
    if f["wide"]:
        return kernel(K_WIDE, pat=use_pat)
    xl_env = sw["RAMD_CSR_XL"]
    if use_pat and xl_env != 0 and f["xl_state"] == 0:
        return ("need", "xl")
    use_xl = use_pat and xl_env != 0 and f["xl_state"] == 1
    grp_env = sw["RAMD_CSR_GRP"]
    if not use_pat and grp_env > 0 and f["grp_state"] == 0 and f["pat_state"] != 1:
        return ("need", "groups")
    use_grp = not use_pat and grp_env != 0 and f["grp_state"] == 1 and not f["pat_off"]
    pat_maxlen = f["pat_maxlen"]
    use_pat2 = use_pat and not use_xl and sw["RAMD_CSR_PAT2"] != 0 and pat_maxlen > 0 and ROWS * pat_maxlen + 3 <= CHUNK
    use_norp = use_pat2 and sw["RAMD_CSR_NORP"] != 0
    col2_env = sw["RAMD_CSR_COL2"]
    col2_candidate = (not use_pat and not use_grp and not (q4_env > 0) and col2_env != 0 and (f["nrow"] >= (1 << 16) or col2_env == 2)
                      and f["nnz"] <= 8 * f["nrow"] and f["blk_span"] >= 0)
    blk_rp = (use_pat2 or use_xl or col2_candidate
              or (sw["RAMD_CSR_BLKRP"] != 0 and not (not use_pat and q4_env > 0) and f["nrow"] >= (1 << 16)))
    if col2_candidate and f["blk_span"] == 0:
        return ("need", "span")
    use_col2 = col2_candidate and f["blk_span"] > 0 and f["blk_span"] <= CHUNK
    use_pipe = sw["RAMD_CSR_PIPE"] != 0
    w4_env = sw["RAMD_CSR_W4"]
    w4_rows = not use_pat and not use_grp and not (q4_env > 0) and not use_col2 and f["nnz"] >= 16 * f["nrow"]
    if w4_rows and w4_env < 0 and f["shift_rows"] < 0:
        return ("need", "shift")
    use_w4 = (not use_pat and not use_grp and not (q4_env > 0) and not use_col2
              and ((w4_env != 0) if w4_env >= 0 else (w4_rows and f["shift_rows"] != 1)))
    lchunk_env = sw["RAMD_CSR_LCHUNK"]
    long_rows = (f["nnz"] >= 16 * f["nrow"] and not use_grp and not (q4_env > 0) and not use_col2 and not use_xl and not use_pat2)
    long_chunk = 0 if not long_rows else (lchunk_env if lchunk_env >= 0 else 4096)
    use_wr = sw["RAMD_CSR_WR"] != 0 and long_rows and long_chunk >= 4096 and not use_w4 and not use_pipe
    wr_gw = sw["RAMD_CSR_WR_GW"]
    gw = 8 if wr_gw == 8 else (14 if wr_gw == 14 else 28)
    w4_waves, wp_env = sw["RAMD_CSR_W4_WAVES"], sw["RAMD_CSR_WP"]
    q4 = not use_pat and q4_env > 0
    # the LAUNCH macro, branch by branch
    if q4:
        return kernel(K_Q4, blk_rp=blk_rp)
    if use_xl:
        return kernel(K_XL, pat=True, blk_rp=blk_rp)
    if use_pat2 and use_norp:
        return kernel(K_PAT2_NORP, pat=True, blk_rp=blk_rp)
    if use_pat2:
        return kernel(K_PAT2, pat=True, blk_rp=blk_rp)
    if use_col2:
        return kernel(K_COL2, blk_rp=blk_rp)
    if use_wr and use_pat:
        return kernel(K_WR, pat=True, gw=gw, blk_rp=blk_rp, wav_rp=True)
    if use_wr:
        return kernel(K_WR, gw=gw, blk_rp=blk_rp, wav_rp=True)
    if use_pat and long_chunk == 8192:
        return kernel(K_TR_PAT, pat=True, chunk=8192, blk_rp=blk_rp)
    if use_pat and long_chunk == 4096:
        return kernel(K_TR_PAT, pat=True, chunk=4096, blk_rp=blk_rp)
    if use_pat:
        return kernel(K_TR_PAT, pat=True, chunk=CHUNK, blk_rp=blk_rp)
    if use_grp:
        return kernel(K_TR_GRP, blk_rp=blk_rp)
    if use_w4 and wp_env != 0 and w4_waves != 1:
        return kernel(K_WP, blk_rp=blk_rp)
    if use_w4 and w4_waves == 1:
        return kernel(K_W4, chunk=1, blk_rp=blk_rp)
    if use_w4:
        return kernel(K_W4, chunk=4, blk_rp=blk_rp)
    if long_chunk >= 4096 and not use_w4:
        return kernel(K_TR, chunk=4096, blk_rp=blk_rp)
    if use_pipe:
        return kernel(K_TR_PIPE, chunk=CHUNK, blk_rp=blk_rp)
    return kernel(K_TR, chunk=CHUNK, blk_rp=blk_rp)


def ell_pick(f, sw):
    """launch_ell; f["nnz"]: nrow * ell_width"""
    pat_env, ell2_env = sw["RAMD_CSR_PAT"], sw["RAMD_ELL2"]
    if f["pat_state"] == 0 and pat_env != 0 and (pat_env > 0 or f["nnz"] >= (1 << 20)):
        return ("need", "patterns")
    use_pat = pat_env != 0 and f["pat_state"] == 1 and not f["pat_off"]
    by_size = (ell2_env != 0) if ell2_env >= 0 else (f["nrow"] >= (1 << 16))
    use2 = use_pat and f["nrow"] % 2 == 0 and f["nrow"] > 0 and by_size
    use2c = not use_pat and f["nrow"] % 2 == 0 and f["nrow"] > 0 and by_size
    if use2:
        return kernel(K_ELL2, pat=True)
    if use2c:
        return kernel(K_ELL2)
    if use_pat:
        return kernel(K_ELL, pat=True)
    return kernel(K_ELL)


def cg_lat_ready(f, sw):
    """csr_cg_lat_ready, but for the arrays it checks (format, lat_vals, pat_id)"""
    patv_switches = (sw["RAMD_CSR_PATV"] != 0 and sw["RAMD_CSR_PAT"] != 0 and sw["RAMD_CSR_XL"] == 0 and sw["RAMD_CSR_PAT2"] != 0
                     and sw["RAMD_CSR_NORP"] == 0)
    lat_admits = sw["RAMD_CSR_LAT"] != 0 and (sw["RAMD_CSR_LAT"] >= 2 or f["nrow"] >= (1 << 16))
    return bool(sw["RAMD_CG_LATDIR"] != 0 and not f["wide"] and f["nnz"] > 0 and f["nrow"] == f["ncol"] and patv_switches
                and f["pat_state"] == 1 and not f["pat_off"] and 0 < f["pat_n"] <= PAT_MAX and f["pat_vstate"] == 1 and f["pat_vdict"]
                and lat_admits and f["lat_state"] == 1)
