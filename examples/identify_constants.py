"""Identify the material constants of the infinite-domain wave case while the net trains: start E, mu, rho away from the values the point
sets were built for and let ``train(identify=...)`` move them -- behind every ``--every``-th Adam step one forward-only call takes the fp64
moment sums of the step's collocation block (pinn_wave2d_material_sums) and a float64 Adam on the host updates (log E, mu, log rho).
The data are the case's own sets: SRC carries (x, y, t) with target (u, v), which is what an identification needs; no further side set.
``--case plate``: the same for the plate with a hole (PINN, plane stress, the reference's E = 20): the distance and particular nets are
pre-trained (or loaded) first, then the composite net trains with identify= on the whole collocation set (pinn_plate2d_material_sums); the
traction on the right edge (RT) is the datum that fixes the stress scale.

    python examples/identify_constants.py --iters 2000 --n-f 20000 --params E mu --E0 3.5 --mu0 0.3
    python examples/identify_constants.py --case plate --iters 500 --n-f 20000 --pre-iters 200 --E0 12 --mu0 0.3      # the plate with a hole
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/identify_constants.py       # data parallel: the sums are all-reduced
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd import pointsets as ps                                      # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import DeepHPM                                 # noqa: E402
from pinn_elastodynamics_amd.plate_hole import PINN                                      # noqa: E402


def plate(a, rank):
    """the plate variant: pre-train (or load) the frozen nets, then Adam on the composite net with identify="""
    c = ps.plate_case(n_collo=a.n_f, n_refine=a.n_f // 2)
    model = PINN(c["Collo"], c["HOLE"], c["IC"], c["LF"], c["RT"], c["UP"], c["LW"], c["DIST"], c["uv_layers"], c["dist_layers"], c["part_layers"],
                 c["lb"], c["ub"], partDir=a.part, distDir=a.dist, uvDir=a.load, precision=a.precision, verbose=False)
    if not a.dist:
        model.train_bfgs_dist(options=dict(maxiter=a.pre_iters, maxfun=a.pre_iters))
    if not a.part:
        model.train_bfgs_part(options=dict(maxiter=a.pre_iters, maxfun=a.pre_iters))
    model.refresh_frozen()
    model.E, model.mu, model.rho = a.E0, a.mu0, a.rho0
    g = model.material_gradient()          # (every rank: the sums are all-reduced across the data-parallel group)
    if rank == 0:
        print("start: E %.4f mu %.4f rho %.4f   dL/dE %.3e dL/dmu %.3e dL/drho %.3e" % (model.E, model.mu, model.rho, g["E"], g["mu"], g["rho"]))
    t0 = time.time()
    hist = model.train(iter=a.iters, learning_rate=a.lr, identify=dict(params=tuple(a.params), lr=a.const_lr, every=a.every))
    if rank == 0:
        print("--- %.1f seconds ---" % (time.time() - t0))
        print("Adam: loss %.4e -> %.4e" % (hist[-1][0], hist[-1][-1]))
        for step, E, mu, rho in model.material_rec[:: max(1, len(model.material_rec) // 10)]:
            print("step %6d  E %.5f  mu %.5f  rho %.5f" % (step, E, mu, rho))
        print("identified: E %.5f mu %.5f rho %.5f" % (model.E, model.mu, model.rho))
        model.save_NN(a.save, TYPE="UV")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="infinite", choices=["infinite", "plate"])
    ap.add_argument("--pre-iters", type=int, default=20000, help="plate: L-BFGS iterations of the distance / particular stages")
    ap.add_argument("--dist", default="", help="plate: weights of the distance net (skips its stage)")
    ap.add_argument("--part", default="", help="plate: weights of the particular net (skips its stage)")
    ap.add_argument("--max-t", type=float, default=20.0)
    ap.add_argument("--n-f", type=int, default=120000)
    ap.add_argument("--width", type=int, default=None, help="hidden width (reference: 80)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch-num", type=int, default=1)
    ap.add_argument("--load", default="", help="weights to start from (reference pickle or .npz)")
    ap.add_argument("--save", default="uv_NN.npz")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--params", nargs="+", default=["E", "mu"], choices=["E", "mu", "rho"], help="the constants to identify")
    ap.add_argument("--E0", type=float, default=3.5, help="starting values (the reference's constants are E = 2.5, mu = 0.25, rho = 1)")
    ap.add_argument("--mu0", type=float, default=0.3)
    ap.add_argument("--rho0", type=float, default=1.0)
    ap.add_argument("--const-lr", type=float, default=1e-3, help="learning rate of the constants' Adam (log E, mu, log rho)")
    ap.add_argument("--every", type=int, default=4, help="identify behind every N-th step: one more forward pass over the block each time")
    a = ap.parse_args()

    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        torch.distributed.init_process_group("nccl")
    rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
    if a.case == "plate":
        plate(a, rank)
        if torch.distributed.is_initialized():
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return

    kw = {} if a.width is None else {"width": a.width}
    c = ps.infinite_case(MAX_T=a.max_t, N_f=a.n_f, **kw)
    model = DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], ExistModel=int(bool(a.load)), modelDir=a.load,
                    case="infinite", precision=a.precision, verbose=rank == 0, E=a.E0, mu=a.mu0, rho=a.rho0)
    if rank == 0:
        g = model.material_gradient()
        print("start: E %.4f mu %.4f rho %.4f   dL/dE %.3e dL/dmu %.3e dL/drho %.3e" % (model.E, model.mu, model.rho, g["E"], g["mu"], g["rho"]))
    else:
        model.material_gradient()          # (every rank: the sums are all-reduced across the data-parallel group)
    t0 = time.time()
    hist = model.train(iter=a.iters, learning_rate=a.lr, batch_num=a.batch_num,
                       identify=dict(params=tuple(a.params), lr=a.const_lr, every=a.every))
    final = model.getloss()
    if rank == 0:
        print("--- %.1f seconds ---" % (time.time() - t0))
        print("Adam: loss %.4e -> %.4e" % (hist[-1][0], hist[-1][-1]))
        for step, E, mu, rho in model.material_rec[:: max(1, len(model.material_rec) // 10)]:
            print("step %6d  E %.5f  mu %.5f  rho %.5f" % (step, E, mu, rho))
        print("identified: E %.5f mu %.5f rho %.5f" % (model.E, model.mu, model.rho))
        print("loss terms on the full sets:", " ".join("%.4e" % v for v in final))
        model.save_NN(a.save)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
