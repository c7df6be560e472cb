"""Causal collocation sampling on the infinite-domain wave case: train with ``train(causal=...)`` -- behind every ``--every``-th Adam step the
time profile of the residual score is taken on ``--probe`` device-drawn points (pinn_wave2d_residual_score, pinn_binned_sums), the causal
weights w_b = exp(-eps * accumulated earlier residual) become a table (pinn_causal_cdf) and this rank's collocation rows are drawn again with
their time coordinate following it (pinn_sample_box_cdf); the source disc is excluded.  Prints the profile, the weights and the rows' time
shares before and after, and the loss terms on the full sets.  ``--eps 0`` leaves the time law uniform (the rows are still redrawn).
Whether this improves a trained field is a question of the method; the script prints what happened and claims nothing.

    python examples/causal_wave.py --iters 2000 --n-f 20000 --eps 1.0 --bins 16 --every 100
    python examples/causal_wave.py --iters 2000 --n-f 20000 --eps 1.0 --refine 200            # with residual-adaptive refinement drawn from the same table
    torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 examples/causal_wave.py    # data parallel: the same table on every rank, no collective
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd import pointsets as ps                                      # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import DeepHPM                                 # noqa: E402


def shares(model, bins):
    """the share of THIS RANK'S collocation rows in each time bin"""
    t = model._collo_host[2][slice(*model._shard(0, model._n_collo))]
    edges = np.linspace(model.lb[2], model.ub[2], bins + 1)
    return np.histogram(t, edges)[0] / max(1, t.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-t", type=float, default=20.0)
    ap.add_argument("--n-f", type=int, default=120000)
    ap.add_argument("--width", type=int, default=None, help="hidden width (reference: 80)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch-num", type=int, default=1)
    ap.add_argument("--load", default="", help="weights to start from (reference pickle or .npz)")
    ap.add_argument("--save", default="uv_NN.npz")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--bins", type=int, default=16, help="time bins of the profile and the table (1 .. 64)")
    ap.add_argument("--eps", type=float, default=1.0, help="causality parameter, in units of 1 / (mean score of the first profile)")
    ap.add_argument("--floor", type=float, default=0.01, help="no bin's density falls below this fraction of the first bin's")
    ap.add_argument("--probe", type=int, default=65536, help="probe points of a profile")
    ap.add_argument("--every", type=int, default=100, help="profile, table and redraw behind every N-th step")
    ap.add_argument("--refine", type=int, default=0, help="also refine behind every N-th step, the candidates drawn from the causal table (0: off)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    if "RANK" in os.environ:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        torch.distributed.init_process_group("nccl")
    rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
    kw = {} if a.width is None else {"width": a.width}
    c = ps.infinite_case(MAX_T=a.max_t, N_f=a.n_f, **kw)
    model = DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], ExistModel=int(bool(a.load)), modelDir=a.load,
                    case="infinite", precision=a.precision, verbose=rank == 0)
    src = [(15.0, 15.0, 2.0)]                                        # the source disc: its points reach scores 1e6 times the median
    fmt = lambda v: " ".join("%.3g" % x for x in v)
    prof, counts = model.residual_profile(a.bins, a.probe, exclude=src, seed=a.seed)
    if rank == 0:
        print("profile before (mean score per time bin):", fmt(prof))
        print("rows' time shares before:               ", fmt(shares(model, a.bins)))
    causal = dict(every=a.every, bins=a.bins, eps=a.eps, floor=a.floor, candidates=a.probe, exclude=src, seed=a.seed)
    refine = dict(every=a.refine, candidates=a.n_f // 4, n_replace=a.n_f // 100, exclude=src, seed=a.seed, causal=True) if a.refine else None
    t0 = time.time()
    if refine is not None:
        # refinement draws from the model's table: make the first one before the loop, for a --refine that comes round before --every does
        model.resample_collocation({k: v for k, v in causal.items() if k != "every"})
    hist = model.train(iter=a.iters, learning_rate=a.lr, batch_num=a.batch_num, causal=causal, refine=refine)
    final = model.getloss()
    out = model.resample_collocation({k: v for k, v in causal.items() if k != "every"})
    if rank == 0:
        print("--- %.1f seconds ---" % (time.time() - t0))
        print("Adam: loss %.4e -> %.4e" % (hist[-1][0], hist[-1][-1]))
        print("profile after:                          ", fmt(out["profile"]))
        print("causal weights w:                       ", fmt(out["w"]))
        print("table (CDF of max(w, floor)):           ", fmt(out["cdf"]))
        print("rows' time shares after the last redraw:", fmt(shares(model, a.bins)))
        print("rows redrawn / kept: %d / %d; score scale of the first profile: %.4g" % (out["redrawn"], out["kept"], getattr(model, "_causal_ref", float("nan"))))
        print("loss terms on the full sets:", " ".join("%.4e" % v for v in final))
        model.save_NN(a.save)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
