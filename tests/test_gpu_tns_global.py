"""BlockJacobi(TNS) on Global objects: 2 ranks on one device (callback transport), CG on the 16^3 Poisson operator.
The preconditioner of the 2-rank run is TNS of every rank's interior block: applied to a fixed vector it gives, bit for bit,
what a TNS plan built on a LocalMatrix of that block gives (every form), and that block is the one numpy cuts out of the whole
operator.  The run converges, held to a numpy CG (tests/_tns_ref.py) whose preconditioner is exactly that block-diagonal
operator: same status, iteration count within the margin CG is granted against its goldens (+-1), same solution."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import _tns_ref as T
from rocalution_amd import distributed as D
from rocalution_amd import generators as gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_jacobi_tns_two_ranks():
    world = 2
    with tempfile.TemporaryDirectory() as d:
        procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_tns_dist_worker.py"), str(r), str(world),
                                   os.path.join(d, "init"), d]) for r in range(world)]
        for p in procs:
            assert p.wait(timeout=300) == 0
        res = [dict(np.load(os.path.join(d, "r%d.npz" % r))) for r in range(world)]
    rp, ci, va = gen.poisson7(16)
    n = len(rp) - 1
    off = D.partition_rows(n, world)
    blocks = []
    for r in range(world):  # the interior block of rank r: its rows, its own columns
        lo, hi = int(off[r]), int(off[r + 1])
        assert (int(res[r]["lo"]), int(res[r]["hi"])) == (lo, hi)
        rows = np.repeat(np.arange(n), np.diff(rp))
        keep = (rows >= lo) & (rows < hi) & (ci >= lo) & (ci < hi)
        brp = np.zeros(hi - lo + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows[keep] - lo, minlength=hi - lo), out=brp[1:])
        blocks.append((lo, hi, brp, ci[keep] - lo, va[keep]))
        # the interior block the rank preconditions is this block ...
        assert np.array_equal(res[r]["irp"], brp) and np.array_equal(res[r]["ici"], ci[keep] - lo)
        assert np.array_equal(res[r]["iva"], va[keep])
        # ... BlockJacobi applies TNS of it bit for bit (auto, stored and matrix-free plans on a LocalMatrix of the block) ...
        zg = res[r]["z_global"]
        for zl in res[r]["z_local"]:
            assert zl.shape == zg.shape and np.array_equal(zl, zg) and np.array_equal(np.signbit(zl), np.signbit(zg))
        # ... and that is TNS: within the forward bound of the longdouble evaluation
        exact = T.tns_apply(brp, ci[keep] - lo, va[keep], res[r]["r"])
        assert np.all(np.abs(zg.astype(T.LD) - exact) <= T.tns_bound(brp, ci[keep] - lo, va[keep], res[r]["r"], 2.0 ** -53))
        assert np.linalg.norm(zg) > 0

    def M(v):
        return np.concatenate([T.tns_apply(brp, bci, bva, v[lo:hi]).astype(np.float64) for lo, hi, brp, bci, bva in blocks])

    A = lambda v: T.csr_matvec(rp, ci, va, v)
    ref_it, ref_st, ref_x, _ = T.cg(A, M, A(np.ones(n)), max_iter=500)
    xs = np.concatenate([r["xs"] for r in res])
    assert ref_st == 2 and int(res[0]["st"]) == 2
    assert abs(int(res[0]["it"]) - ref_it) <= 1, (int(res[0]["it"]), ref_it)
    assert np.linalg.norm(xs - 1.0) / np.sqrt(n) < 1e-5
    assert np.linalg.norm(xs - ref_x) / np.linalg.norm(ref_x) < (1e-8 if int(res[0]["it"]) == ref_it else 1e-5)
