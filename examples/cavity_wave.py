"""Scattering by a cavity: the infinite-domain wave case (INF:634-705) with a traction-free circular cavity beside the source.  The cavity's
surface enters the loss as a traction boundary set -- ``DeepHPM(TRAC=...)``: sigma n = 0 with the per-point normals of
``pointsets.circle_traction_set`` (net_surf_var, INF:267-276; pinn_wave2d_traction_loss_grad) --, the collocation points inside the cavity
are deleted, and refinement and causal sampling keep out of both discs (source and cavity).  Prints every loss term by name, loss_TRAC among
them.  The script poses the problem and prints what happened; it claims nothing about the trained field.

    python examples/cavity_wave.py --iters 2000 --n-f 20000
    python examples/cavity_wave.py --iters 2000 --n-f 20000 --refine 200 --causal 100
    python examples/cavity_wave.py --steps 50                                               # a smoke run: 50 Adam steps on a small set
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd import pointsets as ps                                      # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import DeepHPM                                 # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-t", type=float, default=20.0)
    ap.add_argument("--n-f", type=int, default=120000)
    ap.add_argument("--width", type=int, default=None, help="hidden width (reference: 80)")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=0, help="smoke run: this many Adam steps on 8 000 collocation points, nothing saved")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--cavity", type=float, nargs=3, default=(22.0, 15.0, 1.5), metavar=("XC", "YC", "R"), help="the cavity's disc")
    ap.add_argument("--n-theta", type=int, default=200, help="points on the cavity's surface")
    ap.add_argument("--n-time", type=int, default=100, help="instants of the traction set")
    ap.add_argument("--trac-weight", type=float, default=None, help="multiplier of loss_TRAC in the total (default: that of loss_SRC)")
    ap.add_argument("--refine", type=int, default=0, help="residual-adaptive refinement behind every N-th step (0: off)")
    ap.add_argument("--causal", type=int, default=0, help="causal sampling of the time coordinate behind every N-th step (0: off)")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--save", default="uv_cavity_NN.npz")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    smoke = a.steps > 0
    n_f, iters = (8000, a.steps) if smoke else (a.n_f, a.iters)
    kw = {} if a.width is None else {"width": a.width}
    c = ps.infinite_case(MAX_T=a.max_t, N_f=n_f, N_ext=n_f // 12, **kw)
    xc, yc, r = a.cavity
    Collo = ps.DelSrcPT(c["Collo"], xc, yc, r)                       # no collocation point inside the cavity (the existing helper)
    IC = ps.DelSrcPT(c["IC"], xc, yc, r)
    n_theta, n_time = (40, 25) if smoke else (a.n_theta, a.n_time)
    TRAC = ps.circle_traction_set(xc, yc, r, n_theta, 0.0, a.max_t, n_time)      # unit normals out of the solid, zero traction
    model = DeepHPM(Collo, c["SRC"], IC, c["UP"], c["uv_layers"], c["lb"], c["ub"], case="infinite", precision=a.precision, verbose=not smoke,
                    TRAC=TRAC, trac_weight=a.trac_weight)
    discs = [c["source"], (xc, yc, r)]                                # refinement and causal sampling stay out of both
    refine = dict(every=a.refine, candidates=n_f // 4, n_replace=n_f // 100, exclude=discs, seed=a.seed) if a.refine else None
    causal = dict(every=a.causal, bins=16, eps=1.0, floor=0.01, candidates=min(65536, 4 * n_f), exclude=discs, seed=a.seed) if a.causal else None
    print("collocation %d (inside the cavity removed: %d), SRC %d, IC %d, TRAC %d" % (Collo.shape[0], c["Collo"].shape[0] - Collo.shape[0],
                                                                                       c["SRC"].shape[0], IC.shape[0], TRAC.shape[0]))
    before = model.getloss_dict()
    t0 = time.time()
    hist = model.train(iter=iters, learning_rate=a.lr, batch_num=1, refine=refine, causal=causal)
    after = model.getloss_dict()
    print("--- %d Adam steps, %.1f seconds ---" % (iters, time.time() - t0))
    print("Adam: loss %.4e -> %.4e; loss_TRAC per step %.4e -> %.4e" % (hist[-1][0], hist[-1][-1], model.trac_rec[0], model.trac_rec[-1]))
    for name in sorted(after):
        print("%-10s %.4e -> %.4e" % (name, before[name], after[name]))
    if not smoke:
        model.save_NN(a.save)
    assert np.isfinite(after["loss"]) and np.isfinite(after["loss_TRAC"])


if __name__ == "__main__":
    main()
