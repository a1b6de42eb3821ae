"""csrc/spmv_pick.hpp (the kernel choice of the CSR / ELL products as a pure function) against tests/_spmv_pick_ref.py (the
choice as launch_csr / launch_csr_patv / launch_csr_wide / launch_ell made it before, restated): every answer, the analyses
asked for and their order included, for the default switches, every switch alone at each of its meaningful values, every
setting a test or tool of this repository forces, and a fixed-seed sample of combined settings -- each crossed with a
fixed-seed sample of the fact classes below in which every class occurs.  No GPU: the header is host C++."""
import itertools
import os
import random
import subprocess

import pytest

import _spmv_pick_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEEDS = ["none", "patterns", "values", "lattice", "xl", "groups", "span", "shift"]  # SpmvNeed

ALONE = {"RAMD_CSR_PAT": [0, 1], "RAMD_CSR_PATV": [0, 1], "RAMD_CSR_PATV_LONG": [0, 1], "RAMD_CSR_LAT": [0, 1, 2], "RAMD_CG_LATDIR": [0, 1],
         "RAMD_CSR_Q4": [0, 1], "RAMD_CSR_XL": [0, 1], "RAMD_CSR_GRP": [-1, 0, 1], "RAMD_CSR_PAT2": [0, 1], "RAMD_CSR_NORP": [0, 1],
         "RAMD_CSR_BLKRP": [0, 1], "RAMD_CSR_COL2": [0, 1, 2], "RAMD_CSR_PIPE": [0, 1], "RAMD_CSR_W4": [0, 1], "RAMD_CSR_W4_WAVES": [1, 2, 4],
         "RAMD_CSR_WP": [0, 1], "RAMD_CSR_LCHUNK": [0, 1000, 2048, 4096, 8192], "RAMD_CSR_WR": [0, 1], "RAMD_CSR_WR_GW": [8, 14, 28, 5],
         "RAMD_ELL2": [0, 1]}
# SPMV_VARIANTS of test_gpu_kernels.py (the RAMD_MC_* riders left out), then test_gpu_value_patterns.py, test_gpu_lattice_spmv.py,
# test_gpu_wide_csr.py, test_gpu_lap27.py, test_gpu_cg_lattice_fused.py / test_gpu_cg_x_pairs.py, test_gpu_ellhyb.py /
# _ellhyb_carry.py, tools/cg_interplay.py
FORCED = ["RAMD_CSR_Q4=1", "RAMD_CSR_PAT=1", "RAMD_CSR_PAT=1,RAMD_CSR_XL=1", "RAMD_CSR_PAT=0", "RAMD_CSR_PAT=0,RAMD_CSR_GRP=1",
          "RAMD_CSR_PAT=1,RAMD_CSR_PAT2=0", "RAMD_ELL2=1,RAMD_CSR_PAT=1", "RAMD_ELL2=1,RAMD_CSR_PAT=0", "RAMD_CSR_PAT=0,RAMD_CSR_COL2=2",
          "RAMD_CSR_PAT=1,RAMD_CSR_NORP=1", "RAMD_CSR_PAT=0,RAMD_CSR_W4=1", "RAMD_CSR_PAT=0,RAMD_CSR_W4=1,RAMD_CSR_W4_WAVES=1",
          "RAMD_CSR_PAT=0,RAMD_CSR_W4=1,RAMD_CSR_WP=0", "RAMD_CSR_PAT=0,RAMD_CSR_PIPE=1", "RAMD_CSR_PAT=0,RAMD_CSR_W4=0",
          "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1", "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_PATV_LONG=0", "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_PATV_LONG=1",
          "RAMD_CSR_PAT=1,RAMD_CSR_PATV=0", "RAMD_CSR_PATV=0", "RAMD_CSR_PATV=1",
          "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_LAT=2", "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_LAT=0",
          "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_LAT=2,RAMD_CG_LATDIR=0", "RAMD_CSR_PAT=1,RAMD_CSR_PATV=1,RAMD_CSR_LAT=0,RAMD_CG_LATDIR=0",
          "RAMD_CSR_W4=0", "RAMD_CSR_WR=0", "RAMD_CSR_PAT=1,RAMD_CSR_WR=0", "RAMD_CSR_PAT=1,RAMD_CSR_LAT=2", "RAMD_CSR_PAT2=0", "RAMD_CSR_PAT2=1"]


def _settings():
    out = [""] + ["%s=%d" % (k, v) for k, vs in ALONE.items() for v in vs] + FORCED
    rng = random.Random(20240607)
    for _ in range(120):  # combined: each switch set with probability 1/4, to one of its values or a stray one
        out.append(",".join("%s=%d" % (k, rng.choice(vs + [-1, 3])) for k, vs in ALONE.items() if rng.random() < 0.25))
    return out


# the fact classes: rows below / at 2^16; entries below / at 2^20; mean row length <= 8, between, >= 16; ...
NROW = [300, 65535, 65536, 1 << 18]
MEAN = [4, 8, 12, 16, 20, "2^20-1", "2^20"]
CLASSES = {"pat_state": [0, 1, -1], "pat_off": [0, 1], "pat": [(1, 7), (5, 8), (27, 27), (64, 28), (3, 29), (65, 7), (0, 0)],  # (n, longest)
           "pat_v": [(0, 0), (1, 1), (1, 0), (-1, 0)], "lat_state": [0, 1, -1], "xl_state": [0, 1, -1], "grp_state": [0, 1, -1],
           "blk_span": [0, -1, 2048, 2049], "shift_rows": [-1, 0, 1], "wide": [0, 1], "square": [1, 0]}
assert 256 * 7 + 3 <= 2048 < 256 * 8 + 3  # kCsrRows * len + 3 <= kCsrChunk holds at 7 and fails from 8 on


def _facts(rng, forced):
    """one combination, `forced` = {class: value} fixed (so that every class value occurs), the rest drawn"""
    c = {k: forced.get(k, rng.choice(v)) for k, v in CLASSES.items()}
    nrow, mean = forced.get("nrow", rng.choice(NROW)), forced.get("mean", rng.choice(MEAN))
    nnz = {"2^20-1": (1 << 20) - 1, "2^20": 1 << 20}.get(mean) or nrow * mean
    return dict(nrow=nrow, ncol=nrow if c["square"] else nrow + 5, nnz=nnz, wide=c["wide"], pat_state=c["pat_state"], pat_off=c["pat_off"],
                pat_n=c["pat"][0], pat_maxlen=c["pat"][1], pat_vstate=c["pat_v"][0], pat_vdict=c["pat_v"][1], lat_state=c["lat_state"],
                xl_state=c["xl_state"], grp_state=c["grp_state"], blk_span=c["blk_span"], shift_rows=c["shift_rows"])


def _fact_sample():
    rng = random.Random(7)
    out = [_facts(rng, {k: v}) for k, vs in dict(CLASSES, nrow=NROW, mean=MEAN).items() for v in vs for _ in range(3)]
    # the value-pattern and lattice chain, every state of it, small and large, short and long patterns
    for pv, lat, nrow, pat in itertools.product(CLASSES["pat_v"], CLASSES["lat_state"], [300, 65536], [(1, 7), (27, 27)]):
        out.append(_facts(rng, dict(pat_state=1, pat_off=0, pat=pat, pat_v=pv, lat_state=lat, nrow=nrow, square=1)))
    # matrices that read their columns: every state of the span, shift and group analyses
    for span, shift, grp, mean in itertools.product(CLASSES["blk_span"], CLASSES["shift_rows"], CLASSES["grp_state"], [4, 12, 20]):
        out.append(_facts(rng, dict(pat_state=rng.choice([0, -1]), blk_span=span, shift_rows=shift, grp_state=grp, mean=mean, wide=0)))
    return out + [_facts(rng, {}) for _ in range(150)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spmv_pick") / "spmv_pick_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "drivers", "spmv_pick_driver.cpp"),
                           "-o", exe])
    return exe


def _answer(r):
    return "need %d" % NEEDS.index(r[1]) if r[0] == "need" else "kernel %d %d %d %d %d %d" % r[1:]


def test_header_is_host_only():
    h = open(os.path.join(ROOT, "rocalution_amd", "csrc", "spmv_pick.hpp")).read()
    assert "#include \"" not in h and "#include <hip" not in h


def test_switch_names_and_defaults_agree():
    """every variable the header reads is one the old code read, with the old default; and none is read anywhere else"""
    import re
    h = open(os.path.join(ROOT, "rocalution_amd", "csrc", "spmv_pick.hpp")).read()
    field_of = dict((f, n) for n, f in re.findall(r'\{"(RAMD_\w+)", &s\.(\w+)\}', h))
    defaults = {field_of[f]: int(v) for f, v in re.findall(r"^    int (\w+)\s*= (-?\d+);", h, flags=re.M)}
    assert defaults == ref.DEFAULTS
    for unit in ("spmv.hip", "spmv_wide.hip", "mcsgs.hip"):
        src = open(os.path.join(ROOT, "rocalution_amd", "csrc", unit)).read()
        assert not re.findall(r'getenv\("(RAMD_CSR_\w+|RAMD_ELL2|RAMD_CG_LATDIR)"', src), unit


def test_every_pick_agrees_with_the_restatement(driver):
    settings, facts = _settings(), _fact_sample()
    lines, want = [], []
    for env in settings:
        sw = ref.switches(dict(kv.split("=") for kv in env.split(",") if kv))
        for f in facts:
            ftxt = " ".join(str(int(f[k])) for k in ref.FACTS)
            for mode, dot in ((0, 0), (0, 1), (1, 0), (2, 0)):
                lines.append("%s;%s;0 %d %d" % (env, ftxt, mode, dot)); want.append(_answer(ref.csr_pick(f, sw, mode, dot)))
            lines.append("%s;%s;1 0 0" % (env, ftxt)); want.append(_answer(ref.ell_pick(f, sw)))
            # csr_cg_lat_ready, on the states that occur: the lattice analysis runs only for a matrix whose longest pattern
            # k_csr_patv accepts (under switches that do not change while a process runs), so lattice state 1 with a longer one
            # does not exist and is no case
            if f["lat_state"] != 1 or (0 < f["pat_maxlen"] <= ref.PAT_MAXW
                                       and (256 * f["pat_maxlen"] + 3 <= 2048 or sw["RAMD_CSR_PATV_LONG"] != 0)):
                lines.append("%s;%s;2 0 0" % (env, ftxt)); want.append("ready %d" % ref.cg_lat_ready(f, sw))
    got = subprocess.run([driver], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, text=True).stdout.split("\n")[:-1]
    assert len(got) == len(want) == len(lines) and len(lines) > 100000
    bad = [(l, w, g) for l, w, g in zip(lines, want, got) if w != g]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(lines), bad[:5])
    # every kernel and every analysis occurs among the answers
    assert {w.split()[1] for w in want if w[0] == "k"} == {str(k) for k in range(1, 18)}
    assert {w.split()[1] for w in want if w[0] == "n"} == {str(k) for k in range(1, 8)}
