"""Dev study (GPU): the narrow fused kernels' gradient noise c / sqrt(points) (include/pinn_hip.h PINN_PREC_F16X3 (2), PINN_PREC_BF16X3).
Gradient error against the float64 oracle of the one-stream (data), four-stream (wave) and five-stream (plate) kernels of padded width 64,
4 and 8 hidden layers, bf16x3 and f16x3, fresh Xavier weights, n = 64 / 1024 / 16384, four draws each; the two-kernel path alongside.
Prints one line per draw (error * sqrt(n) is c) and a summary per (head, mode): the constants of the header and of
tests/_variant_matrix.py NARROW_NOISE.   python tools/narrow_noise_study.py"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from pinn_elastodynamics_amd.hip_engine import HipEngine

dev = torch.device("cuda:0")
LB, UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
def rel(a, b): return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
def td(a): return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
rows = []
for head in ("data", "wave", "plate"):
    for prec in ("bf16x3", "f16x3"):
        for depth in (4, 8):
            nout = 5 if head == "plate" else 7
            layers = [3] + depth * [64] + [nout]
            eng = HipEngine(layers, precision=prec, device=dev, max_points=1 << 15)
            for n in (64, 1024, 16384):
                for seed in range(4):
                    rng = np.random.default_rng(100 * seed + n % 97)
                    Ws, bs = po.xavier_init(layers, rng)
                    bs = [0.2 * rng.standard_normal(b.shape) for b in bs]
                    flat = po.pack_params(Ws, bs)
                    th = td(flat)
                    if head == "plate":
                        C = np.stack([rng.random(n) * 0.5, rng.random(n) * 0.5, rng.random(n) * 10], 1)
                        fr = 0.3 * rng.standard_normal((2, 5, 5, n))
                        tw = np.array([10, 7, 13, 9, 11.0]) / n
                        _, g, _ = pl.plate_loss_grad(flat, layers, C[:, 0], C[:, 1], C[:, 2], fr[0], fr[1], term_weights=tw)
                        xs = [td(C[:, k]) for k in range(3)]
                        call = lambda: eng.plate_loss_grad(th, *xs, [0, 0, 0], [0.5, 0.5, 10.0], False, td(fr), tw)[1]
                    else:
                        X = po.collocation_points(n, LB, UB, rng)
                        xs = [td(X[:, k]) for k in range(3)]
                        if head == "data":
                            tg = rng.standard_normal((n, 7))
                            ow = np.array([1, 1, 0, 0, 0, 2, 0.5]) / n
                            _, g, _ = po.data_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], LB, UB, True, tg, ow)
                            call = lambda: eng.data_loss_grad(th, *xs, LB, UB, True, td(tg.T), ow.tolist())[1]
                        else:
                            tw = np.array([1, 2, 3, 1, 0.5, 1, 2.0]) / n
                            _, g, _ = po.wave2d_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], LB, UB, True, term_weights=tw)
                            call = lambda: eng.wave_loss_grad(th, *xs, LB, UB, True, tw)[1]
                    eng.lib.path_counts(reset=True)
                    eng.two_kernel = False
                    gf = call().cpu().numpy()
                    pc = eng.lib.path_counts(reset=True)
                    eng.two_kernel = True
                    g2 = call().cpu().numpy()
                    ef, e2 = rel(gf, g), rel(g2, g)
                    rows.append((head, prec, depth, n, seed, ef, e2, ef * np.sqrt(n)))
                    print(f"{head:5s} {prec:6s} {depth}x64 n={n:6d} seed={seed} fused={ef:.2e} two-kernel={e2:.2e} fused*sqrt(n)={ef*np.sqrt(n):.2e} path={[k for k,v in pc.items() if v]}", flush=True)
from collections import defaultdict
agg = defaultdict(list)
for head, prec, depth, n, seed, ef, e2, c in rows:
    agg[(head, prec)].append(c)
for (head, prec), cs in sorted(agg.items()):
    print(f"{head:5s} {prec:6s}: c mean {np.mean(cs):.2e}, worst {np.max(cs):.2e} ({len(cs)} draws)")
