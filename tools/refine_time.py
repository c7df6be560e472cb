"""Times the refinement calls on one GPU: residual_score beside fields on the same points, select_k beside torch.topk, and score + two selections
beside one training step (loss + gradient + Adam on the same collocation set).  Warm calls, HIP events around each call, medians.
    python tools/refine_time.py [--points 2000000] [--k 200000] [--reps 15] [--out profiles/refine_calls.txt]"""
import argparse
import os
import socket
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd.hip_engine import HipEngine                  # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import xavier_init              # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import pack_params              # noqa: E402


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        for line in out.splitlines():
            if "sclk" in line:
                return line.split(":")[-1].strip()
    except Exception:
        pass
    return "?"


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    layers = [3] + 8 * [64] + [7]
    lb, ub = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
    rng = np.random.default_rng(0)
    W, b = xavier_init(layers, rng)
    theta = torch.from_numpy(pack_params(W, b)).to(dev)
    n = a.points
    x, y, t = (torch.from_numpy((rng.random(n) * u).astype(np.float32)).to(dev) for u in ub)
    eng = HipEngine(layers, precision="f16x3", device=dev, max_points=n)
    tw = [1.0 / n] * 7
    score = eng.residual_score(theta, x, y, t, lb, ub, True, tw)
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    grad, loss = torch.empty_like(theta), torch.empty(8, dtype=torch.float32, device=dev)
    step_no = [0]

    def step():
        step_no[0] += 1
        eng.wave_loss_grad(theta, x, y, t, lb, ub, True, tw, grad_out=grad, loss_out=loss)
        eng.adam_step(theta, m, v, grad, 1e-4, step_no[0])

    def refine():
        s = eng.residual_score(theta, x, y, t, lb, ub, True, tw, out=score)
        eng.select_k(s, a.k, True)
        eng.select_k(s, a.k, False)

    rows = [("fields (28 floats per point)", timed(lambda: eng.fields(theta, x, y, t, lb, ub, True), a.reps)),
            ("residual_score (1 float per point)", timed(lambda: eng.residual_score(theta, x, y, t, lb, ub, True, tw, out=score), a.reps)),
            (f"select_k largest, k = {a.k}", timed(lambda: eng.select_k(score, a.k, True), a.reps)),
            (f"select_k smallest, k = {a.k}", timed(lambda: eng.select_k(score, a.k, False), a.reps)),
            (f"torch.topk (sorted=False), k = {a.k}", timed(lambda: torch.topk(score, a.k, sorted=False), a.reps)),
            ("score + two selections", timed(refine, a.reps)),
            ("training step (wave_loss_grad + adam_step)", timed(step, a.reps))]
    p = torch.cuda.get_device_properties(dev)
    lines = [f"box {socket.gethostname()}: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs, shader clock after the runs: {sclk()}",
             f"net 8 x 64, f16x3, {n} points; median / min / max of {a.reps} warm calls, HIP events around each call [ms]"]
    lines += [f"  {name:48s} {med:9.3f} {lo:9.3f} {hi:9.3f}" for name, (med, lo, hi) in rows]
    d = dict(rows)
    lines.append(f"residual_score / fields = {d['residual_score (1 float per point)'][0] / d['fields (28 floats per point)'][0]:.3f}")
    lines.append(f"(score + two selections) / training step = {d['score + two selections'][0] / d['training step (wave_loss_grad + adam_step)'][0]:.3f}"
                 f"  -> a refinement every 100 steps costs {d['score + two selections'][0] / d['training step (wave_loss_grad + adam_step)'][0]:.2f} % of the steps' time")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
