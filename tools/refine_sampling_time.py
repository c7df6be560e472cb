"""Times one refinement round of DeepHPM (8 x 64, f16x3) on one GPU two ways -- (a) candidates made on the host with pointsets.lhs + DelSrcPT and
passed as an array, generation included (the only route before candidates could be drawn on the device; that path's code is unchanged), (b)
candidates=N drawn on the device, the source disc excluded by keys -- and the parts of (b) and the two new calls alone against their byte counts.
    python tools/refine_sampling_time.py [--points 2000000] [--k 200000] [--rounds 12] [--out profiles/refine_sampling.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd import pointsets                              # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import DeepHPM                   # noqa: E402
from pinn_elastodynamics_amd.hip_engine import HipEngine                   # noqa: E402
from pinn_elastodynamics_amd.refine import pair_by_key                     # noqa: E402

LB, UB, DISC = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0], (15.0, 15.0, 2.0)


def events(fn, reps, warm=3):
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


def wall(fn, rounds, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=200_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, K = a.points, a.k
    layers = [3] + 8 * [64] + [7]
    rng = np.random.default_rng(1111)
    box = lambda m: np.asarray(LB) + (np.asarray(UB) - np.asarray(LB)) * rng.random((m, 3))
    SRC = np.concatenate([box(2000), 0.01 * rng.standard_normal((2000, 2))], 1)
    eng = HipEngine(layers, precision="f16x3", device=dev, max_points=n)
    m = DeepHPM(box(n), SRC, box(2000) * [1, 1, 0], np.zeros((0, 3)), layers, LB, UB, case="infinite", engine=eng, seed=3, verbose=False)
    host_rng = np.random.default_rng(5)
    parts_a = {"gen": [], "del": []}

    def round_host():
        t0 = time.perf_counter()
        C = np.asarray(LB) + pointsets.lhs(3, n, host_rng) * (np.asarray(UB) - np.asarray(LB))
        t1 = time.perf_counter()
        C = pointsets.DelSrcPT(C, *DISC)
        parts_a["gen"].append(1e3 * (t1 - t0))
        parts_a["del"].append(1e3 * (time.perf_counter() - t1))
        return m.refine_collocation(C, K)

    rows = [("(a) host: lhs + DelSrcPT + refine_collocation(array)", wall(round_host, a.rounds))]
    rows.append(("    of it: pointsets.lhs (host)", (statistics.median(parts_a["gen"][2:]), min(parts_a["gen"][2:]), max(parts_a["gen"][2:]))))
    rows.append(("    of it: DelSrcPT (host)", (statistics.median(parts_a["del"][2:]), min(parts_a["del"][2:]), max(parts_a["del"][2:]))))
    for sel in ("top", "sample"):
        rows.append((f"(b) device: refine_collocation({n}, select='{sel}', exclude=[disc])",
                     wall(lambda: m.refine_collocation(n, K, seed=7, select=sel, exclude=[DISC]), a.rounds)))
    # the parts of (b), separate warm calls on the same tensors
    w = m._score_weights(None)
    cand = eng.sample_box(n, LB, UB, 7, 0)
    s_rows, s_cand = m._score_device(m._collo, w), m._score_device(cand, w)
    keys = eng.refine_keys(s_cand, cand, [DISC], "sample", 1.0, 1.0, 7, 0)
    ci, ri = eng.select_k(keys, K).long(), eng.select_k(s_rows, K, largest=False).long()

    def update():
        r, c, _, _ = pair_by_key(ci, keys[ci], s_cand[ci], ri, s_rows[ri])
        for k in range(3):
            m._collo_full[k][r] = cand[k][c]

    rows += [("    draw: sample_box", events(lambda: eng.sample_box(n, LB, UB, 7, 0), 15)),
             ("    score of the rows", events(lambda: m._score_device(m._collo, w), 15)),
             ("    score of the candidates", events(lambda: m._score_device(cand, w, packed=True), 15)),
             ("    keys: refine_keys mask", events(lambda: eng.refine_keys(s_cand, cand, [DISC], "mask"), 15)),
             ("    keys: refine_keys sample", events(lambda: eng.refine_keys(s_cand, cand, [DISC], "sample", 1.0, 1.0, 7, 0), 15)),
             ("    select: two select_k", events(lambda: (eng.select_k(keys, K), eng.select_k(s_rows, K, largest=False)), 15)),
             ("    update: pairing + 3 column scatters", events(update, 15))]
    # the two new calls alone, into preallocated outputs, against the bytes they must move
    cols = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
    kout = torch.empty(n, dtype=torch.float32, device=dev)
    eng.refine_keys(s_cand, cand, [DISC], "mask")                       # (allocates the engine's key workspace)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    ptr = [c.data_ptr() for c in cols]
    cp = [c.data_ptr() for c in cand]
    alone = [("pinn_sample_box, dim 3", 12 * n, lambda: eng.lib.sample_box(7, 0, 0, n, LB, UB, ptr, st())),
             ("pinn_refine_keys mask, 1 disc", 16 * n, lambda: eng.lib.refine_keys(s_cand.data_ptr(), n, cp[0], cp[1], None, [DISC], "mask", 1.0, 1.0, 7, 0, 0,
                                                                                      kout.data_ptr(), eng._keys_ws_ptr, eng._keys_ws_bytes, st())),
             ("pinn_refine_keys sample, 1 disc", 28 * n, lambda: eng.lib.refine_keys(s_cand.data_ptr(), n, cp[0], cp[1], None, [DISC], "sample", 1.0, 1.0, 7,
                                                                                        0, 0, kout.data_ptr(), eng._keys_ws_ptr, eng._keys_ws_bytes, st()))]
    p = torch.cuda.get_device_properties(dev)
    lines = [f"MI355X box: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs",
             f"DeepHPM 8 x 64, f16x3, {n} rows, {n} candidates, n_replace = {K}; median / min / max [ms]",
             f"whole rounds: host clock between two synchronisations, {a.rounds} rounds after 2 warm ones; parts: HIP events, 15 warm calls"]
    lines += [f"  {name:72s} {med:10.3f} {lo:10.3f} {hi:10.3f}" for name, (med, lo, hi) in rows]
    d = dict(rows)
    lines.append(f"(a) / (b, top) = {d[rows[0][0]][0] / d[rows[3][0]][0]:.1f};  (a) / (b, sample) = {d[rows[0][0]][0] / d[rows[4][0]][0]:.1f}")
    lines.append("the new calls alone (preallocated outputs), bytes they must move, achieved rate:")
    for name, nbytes, fn in alone:
        med, lo, hi = events(fn, 30)
        lines.append(f"  {name:40s} {med:8.4f} {lo:8.4f} {hi:8.4f} ms   {nbytes / 1e6:7.1f} MB   {nbytes / med / 1e6:8.1f} GB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
