"""Wall time of the plate's pre-training evaluations (loss_DIST / loss_PART, PLATE:194-215) at the reference's set sizes: the model of
examples/plate_hole.py, its 4 x 20 distance and particular nets.

    python tools/pretrain_time.py [--evals 200] [--warmup 20] [--repeats 5] [--maxfun 500] [--json OUT]

Reports, per stage, the wall time of ``--evals`` calls of PINN._pretrain_loss_grad after ``--warmup`` calls as the median of ``--repeats``
repeats (with min / max: the run-to-run spread), the library calls per evaluation (pinn_debug_path_counts), and the wall time of
train_bfgs_dist(maxfun=--maxfun).  ``--trace-evals N``: nothing but N evaluations of each stage behind the warm-up -- the process to put under
``rocprofv3 --kernel-trace --stats`` for the launches per evaluation.  Works on trees with and without pinn_stream_loss_grad_multi."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                           # noqa: E402
from pinn_elastodynamics_amd import pointsets as ps                    # noqa: E402
from pinn_elastodynamics_amd.plate_hole import PINN                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maxfun", type=int, default=500)
    ap.add_argument("--trace-evals", type=int, default=0)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    c = ps.plate_case(n_collo=4000, n_refine=2000)        # (the collocation set plays no part in the pre-training stages)
    m = PINN(c["Collo"], c["HOLE"], c["IC"], c["LF"], c["RT"], c["UP"], c["LW"], c["DIST"], [3] + 4 * [32] + [5], c["dist_layers"], c["part_layers"],
             c["lb"], c["ub"], verbose=False)
    lib = m.eng["dist"].lib
    stages = (("dist", m._dist_sets), ("part", m._part_sets))
    out = {"set_sizes": {k: [int(s[3]) for s in sets] for k, sets in stages}, "evals": a.evals, "warmup": a.warmup, "repeats": a.repeats,
           "one_call": hasattr(m.eng["dist"], "stream_loss_grad_multi")}
    if a.trace_evals:
        for key, sets in stages:
            for _ in range(a.warmup + a.trace_evals):
                m._pretrain_loss_grad(key, sets)
        torch.cuda.synchronize()
        print(json.dumps({"traced_evals_per_stage": a.warmup + a.trace_evals}))
        return
    for key, sets in stages:
        times = []
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                m._pretrain_loss_grad(key, sets)
            lib.path_counts(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.evals):
                m._pretrain_loss_grad(key, sets)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            calls = lib.path_counts(reset=True)
        out[key] = {"seconds_median": statistics.median(times), "seconds_min": min(times), "seconds_max": max(times), "seconds_all": times,
                    "ms_per_eval_median": 1e3 * statistics.median(times) / a.evals, "library_calls_per_eval": sum(calls.values()) / a.evals, "paths": calls}
    t0 = time.perf_counter()
    res = m.train_bfgs_dist(options=dict(maxiter=a.maxfun, maxfun=a.maxfun))
    out["train_bfgs_dist"] = {"maxfun": a.maxfun, "seconds": time.perf_counter() - t0, "nfev": int(res.nfev), "loss_x1000": float(res.fun)}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
