"""Error of pinn_stream_loss_grad_multi against the float64 oracle at small sets and at trained weights: (a) the fused call, (b) the same
call under PINN_FLAG_TWO_KERNEL, (c) the fp32 mode, at the same points -- the table of profiles/stream_sets_accuracy.txt.

    python tools/stream_sets_accuracy.py > profiles/stream_sets_accuracy.txt

Fresh Xavier 4 x 20 nets on random points and the reference's trained distance / particular nets (tests/golden) on the sets
pointsets.plate_case() builds, 64 / 256 / 1024 points per set and the whole sets."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
from pinn_elastodynamics_amd import pointsets as ps                    # noqa: E402
from tests import _stream_sets as S                                    # noqa: E402


def main():
    dev = torch.device("cuda:0")
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        rev = ""
    print(f"# python tools/stream_sets_accuracy.py    (tree based on commit {rev or 'unknown'}; device {torch.cuda.get_device_name(0)})")
    print("# relative L2 error against the float64 oracle: loss sums / gradient; rule = fused <= max(6 x fp32, 1.5 x two-kernel)")
    print(f"{'case':28s} {'fused':>19s} {'two-kernel':>19s} {'fp32 mode':>19s}  rule")
    layers = [3, 20, 20, 20, 20, 5]
    golden = os.path.join(ROOT, "tests", "golden")
    c = ps.plate_case(n_collo=2000, n_refine=1000)
    for kind in ("dist", "part"):
        patterns = S.DIST_PATTERNS if kind == "dist" else S.PART_PATTERNS
        for n in (64, 256, 1024):
            rng = np.random.default_rng(32)
            flat = S.fresh_net(layers, rng)
            e = S.three_way(layers, flat, S.make_sets(patterns, [n] * len(patterns), rng), dev)
            row(f"fresh {kind} n={n}", e)
        gl, gflat = S.golden_net(golden, kind)
        for n in (64, 256, 1024, None):
            e = S.three_way(gl, gflat, S.case_sets(c, kind, n, np.random.default_rng(33)), dev, max_points=1 << 15)
            row(f"trained {kind} n={n or 'all'}", e)


def row(name, e):
    ok = all(e["fused"][i] <= max(6.0 * e["fp32"][i], 1.5 * e["two-kernel"][i]) for i in (0, 1))
    print(f"{name:28s} " + " ".join(f"{e[k][0]:9.2e}/{e[k][1]:9.2e}" for k in ("fused", "two-kernel", "fp32")) + ("  ok" if ok else "  MISSED"), flush=True)


if __name__ == "__main__":
    main()
