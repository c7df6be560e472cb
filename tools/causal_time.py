"""Times the causal-sampling calls on one GPU and what train(causal=...) costs.
  calls   sample_box(t_cdf=...) beside sample_box, binned_sums (64 bins) beside field_error_sums and residual_score at the same n, causal_cdf
          alone: 5 warm-up calls, three alternated rounds of 30 calls per kind, HIP events around each call, median / min / max per round.
  train   DeepHPM.train at 8 x 64, f16x3, on --points collocation points, ms per step: wall clock around train(100 steps) between device
          synchronisations, 20 warm-up steps, --rounds timed calls.  One process per run; ``--tree`` runs ANOTHER checkout's package (the parent
          commit, built in a directory of its own) the same way, ``--causal`` omit | none | every100.
  all     calls, then --runs alternated train runs of each of: the --tree checkout (keyword omitted), this tree with causal=None, this tree
          with causal=dict(every=100, candidates=65536), each in a fresh child process.
    python tools/causal_time.py all --tree ../parent-checkout --out profiles/causal_calls.txt"""
import argparse
import os
import socket
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        for line in out.splitlines():
            if "sclk" in line:
                return line.split(":")[-1].strip()
    except Exception:
        pass
    return "?"


def rounds_of(kinds, reps=30, rounds=3, warm=5):
    """{name: [(median, min, max) per round]} of the callables in ``kinds``, the kinds alternated inside every round"""
    import torch
    for fn in kinds.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in kinds}
    for _ in range(rounds):
        for name, fn in kinds.items():
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            out[name].append((statistics.median(ms), min(ms), max(ms)))
    return out


def calls(a):
    import numpy as np
    import torch
    sys.path.insert(0, HERE)
    from pinn_elastodynamics_amd.elastic_wave import pack_params, xavier_init
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    dev = torch.device("cuda:0")
    layers = [3] + 8 * [64] + [7]
    lb, ub = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
    rng = np.random.default_rng(0)
    theta = torch.from_numpy(pack_params(*xavier_init(layers, rng))).to(dev)
    n = a.calls_points
    eng = HipEngine(layers, precision="f16x3", device=dev, max_points=n)
    x, y, t = eng.sample_box(n, lb, ub, 1)
    tw = [1.0] * 7
    score = eng.residual_score(theta, x, y, t, lb, ub, True, tw)
    binned = eng.binned_sums(score, t, lb[2], ub[2], 64)
    w, cdf = eng.causal_cdf(binned, 1.0 / float(score.mean()), 0.01)
    pred = torch.randn((8, n), dtype=torch.float32, device=dev)
    ref5, ref1 = pred[:5].clone() + 0.1, pred[:1].clone() + 0.1
    kinds = {
        "sample_box (3 columns)": lambda: eng.sample_box(n, lb, ub, 1),
        "sample_box(t_cdf), 64 bins": lambda: eng.sample_box(n, lb, ub, 1, t_cdf=cdf),
        "binned_sums, 64 bins": lambda: eng.binned_sums(score, t, lb[2], ub[2], 64, out=binned),
        "binned_sums, 16 bins": lambda: eng.binned_sums(score, t, lb[2], ub[2], 16),
        "field_error_sums, 1 row": lambda: eng.field_error_sums(pred, (0,), ref1),
        "field_error_sums, 5 rows": lambda: eng.field_error_sums(pred, (0, 1, 2, 3, 4), ref5),
        "residual_score 8 x 64": lambda: eng.residual_score(theta, x, y, t, lb, ub, True, tw, out=score),
        "causal_cdf, 64 bins": lambda: eng.causal_cdf(binned, 1.0, 0.01),
    }
    p = torch.cuda.get_device_properties(dev)
    clk0 = sclk()
    res = rounds_of(kinds)
    lines = [f"box {socket.gethostname()}: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs; shader clock before / after the runs: {clk0} / {sclk()}",
             f"f16x3, {n} points; HIP events around each call, 5 warm-up calls, three alternated rounds of 30 calls per kind; median/min/max of each round [ms]",
             "(the sample_box and binned_sums rows include the allocation of their outputs by the caching allocator, as the engine calls do)"]
    for name, r in res.items():
        lines.append(f"  {name:30s} " + "   ".join("%.4f/%.4f/%.4f" % v for v in r))
    med = {k: statistics.median(v[0] for v in r) for k, r in res.items()}
    lines.append(f"sample_box(t_cdf) / sample_box = {med['sample_box(t_cdf), 64 bins'] / med['sample_box (3 columns)']:.2f}; "
                 f"binned_sums (64) / field_error_sums (1 row) = {med['binned_sums, 64 bins'] / med['field_error_sums, 1 row']:.2f}; "
                 f"binned_sums (64) / residual_score = {med['binned_sums, 64 bins'] / med['residual_score 8 x 64']:.3f}")
    lines.append(f"bytes moved at {n} points: sample_box writes {12 * n / 1e6:.0f} MB, binned_sums reads {8 * n / 1e6:.0f} MB -> "
                 f"{12 * n / 1e6 / med['sample_box(t_cdf), 64 bins']:.0f} GB/s and {8 * n / 1e6 / med['binned_sums, 64 bins']:.0f} GB/s over the median call time")
    return lines


def train(a):
    tree = os.path.abspath(a.tree) if a.tree else HERE
    sys.path.insert(0, tree)
    import torch
    from pinn_elastodynamics_amd import pointsets as ps
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    c = ps.infinite_case(MAX_T=20.0, N_f=a.points, width=64)
    m = DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], case="infinite", precision="f16x3", verbose=False)
    kw = {"omit": {}, "none": {"causal": None},
          "every100": {"causal": dict(every=100, bins=64, eps=1.0, candidates=65536, exclude=[(15.0, 15.0, 2.0)])}}[a.causal]
    m.train(20, 1e-4, 1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        m.train(100, 1e-4, 1, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 10.0)
    print("RESULT %s %s layers=%s n=%d sides=%d+%d median %.3f [%s]" % (
        "parent" if a.tree else "this", a.causal, "x".join(str(v) for v in c["uv_layers"]), m._n_collo, len(c["SRC"]), len(c["IC"]), statistics.median(ms),
        " ".join("%.3f" % v for v in ms)), flush=True)


def everything(a):
    lines = ["==== 1. call time"] + calls(a)
    lines += ["", f"==== 2. cost in training (same box and session; DeepHPM.train, case infinite, 8 x 64, f16x3, {a.points} collocation points, one block; wall "
              "clock around train(100 steps) between device synchronisations, 20 warm-up steps, one fresh process per run, the runs alternated; ms per "
              "step, median [all timed calls])"]
    runs = [("omit", a.tree), ("none", ""), ("every100", "")]
    for r in range(a.runs):
        for causal, tree in runs:
            if causal == "omit" and not tree:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "train", "--points", str(a.points), "--rounds", str(a.rounds), "--causal", causal]
            out = subprocess.run(cmd + (["--tree", tree] if tree else []), capture_output=True, text=True, timeout=900)
            got = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
            if out.returncode != 0 or not got:              # a child that failed ends the session: nothing more is started on the device
                lines.append(f"  run {r} {causal}: child failed with status {out.returncode}: {out.stderr[-500:]}")
                return lines, 1
            lines.append(f"  run {r}  " + got[0][7:])
            print(lines[-1], flush=True)
    lines.append(f"shader clock after the runs: {sclk()}")
    return lines, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["calls", "train", "all"])
    ap.add_argument("--calls-points", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tree", default="", help="another checkout of the package (the parent commit, built) to time the same way")
    ap.add_argument("--causal", default="none", choices=["omit", "none", "every100"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "train":
        return train(a)
    lines, rc = (calls(a), 0) if a.mode == "calls" else everything(a)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.exit(rc)


if __name__ == "__main__":
    main()
