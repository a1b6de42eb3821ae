"""Worker of the 2-rank TNS test (tests/test_gpu_tns_global.py): CG + BlockJacobi(TNS) on Global objects, the ranks sharing one
device over the host-staged callback transport.  Every rank also applies the built preconditioner to a fixed vector and, for
comparison, TNS plans built on a LocalMatrix of its interior block."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(rank, world, initfile, outdir):
    import _dist_worker as W
    import rocalution_amd as ra
    from rocalution_amd import capi, distributed as D, generators as gen
    dist = W._init(rank, world, initfile)
    ra.init_rocalution(0)
    comm = D.make_callback_comm(rank, world, dist)
    rp, ci, va = gen.poisson7(16)
    n = len(rp) - 1
    off = D.partition_rows(n, world)
    piece = D.split_rows(rp, ci, va, off, rank)
    plan = D.build_halo_plan(piece, off, rank, W._gather_obj(dist, world))
    lo, hi = piece["row_begin"], piece["row_end"]
    g = D.DistributedSolver(comm, capi.SOLVER_CG, capi.PC_TNS)
    g.setup_csr(n, piece, plan)
    g.init(1e-15, 1e-6, 1e8, 500)
    g.build()
    # the preconditioner on a fixed right-hand side, next to TNS plans built on a LocalMatrix of this rank's interior block
    from rocalution_amd import solvers as S
    r = np.random.default_rng(77).uniform(-1.0, 1.0, n)[lo:hi]
    z_global = g.precond_apply(r)
    irp, ici, iva = piece["interior"]
    B = ra.LocalMatrix()
    B.SetDataPtrCSR(irp, ici, iva, nrow=hi - lo, ncol=hi - lo)
    z_local = []
    for form in (-1, 0, 1):
        plan = S.TNSPlan(B, form=form)
        x = ra.LocalVector(); x.Allocate("", hi - lo)
        plan.Apply(ra.LocalVector(data=r), x)
        z_local.append(x.numpy())
    xs = g.solve(None, np.zeros(hi - lo))
    it, st, res = g.result()
    np.savez(os.path.join(outdir, "r%d.npz" % rank), lo=lo, hi=hi, it=it, st=st, res=res, xs=xs, r=r, z_global=z_global,
             z_local=np.array(z_local), irp=irp, ici=ici, iva=iva)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4])
