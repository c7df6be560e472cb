"""Evaluations per second of the L-BFGS stages under the three optimizers (backend = scipy | torch | hip), in one session.

    python tools/lbfgs_stage_time.py [--maxfun 300] [--rounds 2] [--stages plate,dist,part,inf] [--out profiles/lbfgs_device_ab.txt]
    python tools/lbfgs_stage_time.py --trace-stage dist --history 50 --maxfun 200      # one hip stage, for rocprofv3 --kernel-trace --stats

Stages: the plate's main stage at the reference's sizes (uv 8 x 70, PLATE:885), its two pre-training stages (4 x 20 nets) and the INF wave stage
(8 x 80, INF:645).  Every stage starts from the same fresh weights under each backend; the backends are interleaved (scipy, torch, hip, scipy,
...) over ``--rounds`` rounds behind one short warm-up run of EVERY backend, and the shader clock is read before each run.  A rate is function evaluations / wall second
of the train_bfgs* call, host work included -- what a user waits for."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from pinn_elastodynamics_amd import pointsets as ps                    # noqa: E402


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        for line in out.splitlines():
            if "sclk" in line:
                return line.split(":")[-1].strip()
    except Exception:
        pass
    return "?"


def plate_model():
    from pinn_elastodynamics_amd.plate_hole import PINN
    c = ps.plate_case()
    return PINN(c["Collo"], c["HOLE"], c["IC"], c["LF"], c["RT"], c["UP"], c["LW"], c["DIST"], c["uv_layers"], c["dist_layers"], c["part_layers"],
                c["lb"], c["ub"], verbose=False)


def wave_model():
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    c = ps.infinite_case()                                   # INF:634-705: 8 x 80, ~130 k collocation points
    return DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], case="infinite", verbose=False)


def run_stage(stage, backend, maxfun, history):
    opts = dict(maxiter=maxfun, maxfun=maxfun, maxcor=history)
    if stage == "inf":
        m = wave_model()
        call = lambda: m.train_bfgs(1, options=opts, backend=backend)
    else:
        m = plate_model()
        call = {"plate": lambda: m.train_bfgs(options=opts, backend=backend), "dist": lambda: m.train_bfgs_dist(options=opts, backend=backend),
                "part": lambda: m.train_bfgs_part(options=opts, backend=backend)}[stage]
    m.verbose = False
    n0 = m.count
    torch.cuda.synchronize()
    clk = sclk()
    t0 = time.perf_counter()
    res = call()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nfev = m.count - n0
    return dict(stage=stage, backend=backend, nfev=int(nfev), seconds=dt, evals_per_s=nfev / dt, ms_per_eval=1e3 * dt / max(1, nfev), fun=float(res["fun"] if isinstance(res, dict) else res.fun),
                sclk=clk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maxfun", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--history", type=int, default=50)
    ap.add_argument("--stages", default="plate,dist,part,inf")
    ap.add_argument("--backends", default="scipy,torch,hip")
    ap.add_argument("--trace-stage", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.trace_stage:
        print(json.dumps(run_stage(a.trace_stage, "hip", a.maxfun, a.history)))
        return
    lines = [f"# L-BFGS stage rates: maxfun {a.maxfun}, history {a.history}, {a.rounds} interleaved rounds; {torch.cuda.get_device_name(0)}"]
    rows = []
    for stage in a.stages.split(","):
        for backend in a.backends.split(","):                 # warm every backend's first-run costs (kernels, allocator, torch's optimizer)
            run_stage(stage, backend, 20, a.history)
        for r in range(a.rounds):
            for backend in a.backends.split(","):
                row = run_stage(stage, backend, a.maxfun, a.history)
                row["round"] = r
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    lines.append("# best of the rounds: stage backend evals/s ms/eval")
    for stage in a.stages.split(","):
        for backend in a.backends.split(","):
            best = max((x for x in rows if x["stage"] == stage and x["backend"] == backend), key=lambda x: x["evals_per_s"])
            lines.append(f"{stage:6s} {backend:6s} {best['evals_per_s']:9.1f} {best['ms_per_eval']:8.3f}")
            print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
