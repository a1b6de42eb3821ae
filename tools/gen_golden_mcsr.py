"""Record the genuine rocALUTION library's MCSR conversions, products and CG + Jacobi solve for tests/golden/mcsr/*.npz.

    python tools/gen_golden_mcsr.py [outdir]

Compiles tests/drivers/mcsr_probe.cpp (public header and installed library only, accelerator disabled, one OpenMP thread)
into a temporary directory, runs it on the operators below and writes one .npz per operator.  Every file holds the input CSR
(rowptr, col, val), x and y of the products, `format` (2, or 1 where the library refuses) and, where it converts:
mcsr_rowptr / _col / _val (LeaveDataPtrMCSR), spmv_mcsr = A x, spmv_mcsr_add = y - 0.75 A x (ApplyAdd), back_rowptr / _col /
_val (converted back to CSR); the fp32 run's values as mcsr_val_f32, spmv_mcsr_f32, spmv_mcsr_add_f32, back_val_f32 (the
script checks that its integer arrays equal the fp64 run's).  The solver fixtures add rhs and cg_jacobi_mcsr_{meta,hist,x}:
CG + Jacobi with the library's default tolerances on the operator converted to MCSR before Build().  `csr_differs` is the
number of elements in which spmv_mcsr differs from the CSR loop's sum (tests/_mcsr_ref.py csr_apply) on the same x, in fp64
and fp32: where it is 0 the archive could not tell the diagonal-first order from CSR's, and for the operators of DIFFER the
script draws another x until it is not.  The archives are written with a fixed time stamp: a second run gives the same bytes.

The operators:
  gr3030, poisson8, lap2d7, lap27_6, rand300, rand300ell   the CSR, x, y and rhs_ones of tests/golden/<name>.npz: sorted rows,
                  a full diagonal (checked here).  gr3030 and poisson8 are the solver fixtures.
  shuffled_257, longrow, hub, zeros_64, negzero_64, nodiag_row_40   of tests/_mcsr_cases.py, with a uniform x in [-1, 1) (the
                  tests' dyadic x makes every sum exact, in any order) except negzero_64, whose signed zeros are the point.
                  nodiag_row_40 records the refusal.
"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mcsr_cases as cases  # noqa: E402
import _mcsr_ref as ref  # noqa: E402
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FIXTURES = ["gr3030", "poisson8", "lap2d7", "lap27_6", "rand300", "rand300ell"]
SOLVE = ["gr3030", "poisson8"]
GENERATED = ["shuffled_257", "longrow", "hub", "zeros_64", "negzero_64", "nodiag_row_40"]
DIFFER = ["gr3030", "shuffled_257"]


def save(path, d):
    """np.savez_compressed with a fixed time stamp and key order"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def inputs(name, attempt):
    """-> (rp, ci, va, x, y, rhs or None)"""
    if name in FIXTURES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        rp, ci, va = g["rowptr"].astype(np.int32), g["col"].astype(np.int32), g["val"].astype(np.float64)
        n = len(rp) - 1
        for r in range(n):
            cols = ci[rp[r]:rp[r + 1]]
            assert np.all(np.diff(cols) > 0) and r in cols, (name, r)
        x = g["x"] if attempt == 0 else np.random.default_rng(1000 + attempt).uniform(-1.0, 1.0, n)
        return rp, ci, va, x.astype(np.float64), g["y"].astype(np.float64), g["rhs_ones"] if name in SOLVE else None
    rp, ci, va = cases.case(name)
    n = len(rp) - 1
    x = cases.x_for(name) if name == "negzero_64" else np.random.default_rng(2000 + 17 * attempt + len(name)).uniform(-1.0, 1.0, n)
    return rp, ci, va, x, cases.y_for(name), None


def _read(outd):
    out = {}
    for f in sorted(os.listdir(outd)):
        p = os.path.join(outd, f)
        if f.endswith("_hist.txt"):
            out[f[:-4]] = np.array([float(s) for s in open(p).read().split()])
            continue
        key = f[:-4]
        if key.startswith("format") or key.endswith(("_rowptr", "_col", "_rowptr_f32", "_col_f32")):
            dt = np.int32
        elif key.endswith("_f32"):
            dt = np.float32
        else:
            dt = np.float64
        out[key] = np.fromfile(p, dtype=dt)
    return out


def record(exe, tmp, name):
    for attempt in range(20):
        rp, ci, va, x, y, rhs = inputs(name, attempt)
        ind, outd = os.path.join(tmp, "%s_in%d" % (name, attempt)), os.path.join(tmp, "%s_out%d" % (name, attempt))
        os.makedirs(ind); os.makedirs(outd)
        np.array([len(rp) - 1, len(ci)], dtype=np.int64).tofile(os.path.join(ind, "hdr.bin"))
        for f, a in (("rowptr", rp), ("col", ci), ("val", va), ("x", x), ("y", y), ("rhs", rhs if rhs is not None else np.zeros(0))):
            a.tofile(os.path.join(ind, f + ".bin"))
        subprocess.check_call([exe, ind, outd] + (["solve"] if rhs is not None else []), env=dict(os.environ, OMP_NUM_THREADS="1"),
                              stdout=subprocess.DEVNULL)
        raw = _read(outd)
        d = {"rowptr": rp, "col": ci, "val": va, "x": x, "y": y, "format": raw["format"]}
        assert np.array_equal(raw["format"], raw["format_f32"]), name
        if int(raw["format"][0]) != 2:
            return d
        for k, v in raw.items():
            if k.startswith("format"):
                continue
            if k.endswith("_f32"):
                if k.endswith("_val_f32") or k.startswith("spmv"):
                    d[k] = v
                else:
                    assert np.array_equal(v, raw[k[:-4]]), (name, k)
            else:
                d[k] = v
        if rhs is not None:
            assert int(raw["format_after_solve"][0]) == 2, name
            d["rhs"] = rhs
        differs = []
        for sfx, t, u in (("", np.float64, np.uint64), ("_f32", np.float32, np.uint32)):
            c = ref.csr_apply(rp, ci, va.astype(t), x.astype(t))
            differs.append(int(np.sum(d["spmv_mcsr" + sfx].view(u) != c.view(u))))
        d["csr_differs"] = np.array(differs, np.int64)
        if name not in DIFFER or min(differs) > 0:
            return d
    raise RuntimeError(name + ": no x found on which the MCSR product differs from the CSR product")


def main():
    outdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "mcsr")
    os.makedirs(outdir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "mcsr_probe")
        subprocess.check_call(["g++", "-O2", "-fopenmp", "-I" + os.path.join(ROCM, "include"),
                               os.path.join(ROOT, "tests", "drivers", "mcsr_probe.cpp"), "-L" + os.path.join(ROCM, "lib"),
                               "-lrocalution", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
        for name in FIXTURES + GENERATED:
            d = record(exe, tmp, name)
            path = os.path.join(outdir, name + ".npz")
            save(path, d)
            print(name, os.path.getsize(path), "bytes; format", int(d["format"][0]),
                  "; differs from CSR in", d["csr_differs"].tolist() if "csr_differs" in d else "-",
                  "; CG iterations", int(d["cg_jacobi_mcsr_meta"][0]) if "cg_jacobi_mcsr_meta" in d else "-")


if __name__ == "__main__":
    main()
