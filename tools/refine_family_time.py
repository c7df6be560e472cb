"""Times the refinement calls of the plate and 3-D families on one GPU: plate_residual_score / nc3d_residual_score beside the route they replace
(net_streams / nc3d_fields, then the composite and residual formulas of the model classes in torch on the device), and one refine_collocation of
PINN and of NavierCauchy3D with its parts timed one by one.  Warm calls, HIP events around each call, medians.
    python tools/refine_family_time.py [--points 1000000] [--rows 500000] [--replace 25000] [--reps 15] [--out profiles/refine_family_calls.txt]"""
import argparse
import os
import socket
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd.elastic_wave import pack_params, xavier_init                  # noqa: E402
from pinn_elastodynamics_amd.hip_engine import HipEngine                                   # noqa: E402
from pinn_elastodynamics_amd.navier_cauchy_3d import NavierCauchy3D, halfspace_case        # noqa: E402
from pinn_elastodynamics_amd.plate_hole import PINN                                        # noqa: E402
from pinn_elastodynamics_amd.refine import pair_replacements                               # noqa: E402
from tools.refine_time import sclk, timed                                                  # noqa: E402

DEV = torch.device("cuda:0")
P_LB, P_UB = [0.0, 0.0, 0.0], [0.5, 0.5, 10.0]
N_LB, N_UB = [0.0, 0.0, -30.0, 0.0], [30.0, 30.0, 0.0, 15.0]


def net(layers, seed=0):
    W, b = xavier_init(layers, np.random.default_rng(seed))
    return torch.from_numpy(pack_params(W, b)).to(DEV)


def cols(n, lb, ub, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy((lo + (hi - lo) * rng.random(n)).astype(np.float32)).to(DEV) for lo, hi in zip(lb, ub)]


def plate_torch_route(eng, th, xs, fr, w, E=20.0, mu=0.25, rho=1.0):
    """net_streams of the uv net, then PINN._composite / net_f_sig (plate_hole.py) and the weighted sum of squares, in torch on the device"""
    N, D, P = eng.net_streams(th, *xs, P_LB, P_UB, False), fr[0], fr[1]
    F = torch.empty_like(N)
    F[0] = P[0] + D[0] * N[0]
    for k in (1, 2, 3):
        F[k] = P[k] + D[k] * N[0] + D[0] * N[k]
    F[4] = P[4] + D[4] * N[0] + 2.0 * D[3] * N[3] + D[0] * N[4]
    e11, e22, e12 = F[1, 0], F[2, 1], F[2, 0] + F[1, 1]
    sp11 = E / (1 - mu * mu) * e11 + E * mu / (1 - mu * mu) * e22
    sp22 = E * mu / (1 - mu * mu) * e11 + E / (1 - mu * mu) * e22
    sp12 = E / (2 * (1 + mu)) * e12
    f = torch.stack([F[1, 2] + F[2, 4] - rho * F[4, 0], F[2, 3] + F[1, 4] - rho * F[4, 1], F[0, 2] - sp11, F[0, 3] - sp22, F[0, 4] - sp12])
    return (w[:, None] * f * f).sum(0)


def nc3d_torch_route(eng, th, xs, w, E=2.5, mu=0.25, rho=1.0):
    """nc3d_fields, then NavierCauchy3D.net_f_sig (navier_cauchy_3d.py) and the weighted sum of squares, in torch on the device"""
    F = eng.nc3d_fields(th, *xs, N_LB, N_UB, True)
    V, X, Y, Z, T = F[0], F[1], F[2], F[3], F[4]
    coef = E / ((1 + mu) * (1 - 2 * mu))
    c1, c2, G = coef * (1 - mu), coef * mu, E / (2 * (1 + mu))
    e11, e22, e33 = X[0], Y[1], Z[2]
    e12, e13, e23 = Y[0] + X[1], Z[0] + X[2], Z[1] + Y[2]
    f = [X[6] + Y[9] + Z[10] - rho * T[3], X[9] + Y[7] + Z[11] - rho * T[4], X[10] + Y[11] + Z[8] - rho * T[5],
         T[0] - V[3], T[1] - V[4], T[2] - V[5],
         V[6] - (c1 * e11 + c2 * (e22 + e33)), V[7] - (c1 * e22 + c2 * (e11 + e33)), V[8] - (c1 * e33 + c2 * (e11 + e22)),
         V[9] - G * e12, V[10] - G * e13, V[11] - G * e23]
    f = torch.stack(f)
    return (w[:, None] * f * f).sum(0)


def fmt(rows):
    return [f"  {name:64s} {med:9.3f} {lo:9.3f} {hi:9.3f}" for name, (med, lo, hi) in rows]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=500_000)
    ap.add_argument("--replace", type=int, default=25_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, R, K = a.points, a.rows, a.replace
    p = torch.cuda.get_device_properties(DEV)
    lines = [f"box {socket.gethostname()}: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs",
             f"f16x3; median / min / max of {a.reps} warm calls, HIP events around each call [ms]"]

    # ---- plate: 8 x 64 uv net, frozen streams resident
    lN = [3] + 8 * [64] + [5]
    eng, th, xs = HipEngine(lN, precision="f16x3", device=DEV, workspace_bytes=0), net(lN), cols(n, P_LB, P_UB, 1)
    fr = (torch.randn((2, 5, 5, n), device=DEV) * torch.tensor([1.0, 2.0, 2.0, 0.2, 0.05], device=DEV)[None, :, None, None]).contiguous()
    w = [10.0] * 5
    wt = torch.tensor(w, device=DEV)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    s_new, s_old = eng.plate_residual_score(th, *xs, P_LB, P_UB, False, fr, w, out=out), plate_torch_route(eng, th, xs, fr, wt)
    agree = float(((s_new - s_old).abs() / s_old.abs().clamp_min(1e-30)).max())
    rows = [("plate_residual_score (1 float per point)", timed(lambda: eng.plate_residual_score(th, *xs, P_LB, P_UB, False, fr, w, out=out), a.reps)),
            ("net_streams (25 floats per point) alone", timed(lambda: eng.net_streams(th, *xs, P_LB, P_UB, False), a.reps)),
            ("net_streams + composite and residuals in torch (the route replaced)", timed(lambda: plate_torch_route(eng, th, xs, fr, wt), a.reps))]
    lines += [f"plate, uv net 8 x 64, {n} points (largest relative difference of the two routes' scores: {agree:.1e})"] + fmt(rows)
    lines.append(f"  plate_residual_score / replaced route = {rows[0][1][0] / rows[2][1][0]:.3f}")
    del fr, s_new, s_old, out
    torch.cuda.empty_cache()

    # ---- 3-D: 10 x 128
    l3 = [4] + 10 * [128] + [12]
    eng3, th3, xs3 = HipEngine(l3, precision="f16x3", device=DEV, workspace_bytes=0), net(l3), cols(n, N_LB, N_UB, 2)
    w3 = [5.0] * 12
    wt3 = torch.tensor(w3, device=DEV)
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    s_new, s_old = eng3.nc3d_residual_score(th3, *xs3, N_LB, N_UB, True, w3, out=out), nc3d_torch_route(eng3, th3, xs3, wt3)
    agree = float(((s_new - s_old).abs() / s_old.abs().clamp_min(1e-30)).max())
    rows = [("nc3d_residual_score (1 float per point)", timed(lambda: eng3.nc3d_residual_score(th3, *xs3, N_LB, N_UB, True, w3, out=out), a.reps)),
            ("nc3d_fields (60 floats per point) alone", timed(lambda: eng3.nc3d_fields(th3, *xs3, N_LB, N_UB, True), a.reps)),
            ("nc3d_fields + residuals in torch (the route replaced)", timed(lambda: nc3d_torch_route(eng3, th3, xs3, wt3), a.reps))]
    lines += [f"3-D, net 10 x 128, {n} points (largest relative difference of the two routes' scores: {agree:.1e})"] + fmt(rows)
    lines.append(f"  nc3d_residual_score / replaced route = {rows[0][1][0] / rows[2][1][0]:.3f}")
    del s_new, s_old, out, xs, xs3
    torch.cuda.empty_cache()

    # ---- one refine_collocation of each class, and its parts
    rng = np.random.default_rng(5)
    box = lambda m, lb, ub: np.asarray(lb) + (np.asarray(ub) - np.asarray(lb)) * rng.random((m, len(lb)))
    side = lambda m, fix: box(m, P_LB, P_UB) * fix[0] + fix[1]              # (a boundary set: one coordinate pinned)
    zero = np.zeros(3)
    HOLE = np.stack([0.1 * np.cos(np.linspace(0, 1.5, 64)), 0.1 * np.sin(np.linspace(0, 1.5, 64)), np.linspace(0, 10, 64)], 1)
    IC, LF = side(64, (np.array([1, 1, 0]), zero)), side(64, (np.array([0, 1, 1]), zero))
    RT = np.concatenate([side(64, (np.array([0, 1, 1]), np.array([0.5, 0, 0]))), rng.random((64, 1))], 1)
    UP, LW = side(64, (np.array([1, 0, 1]), np.array([0, 0.5, 0]))), side(64, (np.array([1, 0, 1]), zero))
    DIST = np.concatenate([box(64, P_LB, P_UB), rng.random((64, 5))], 1)
    lS = [3] + 4 * [20] + [5]
    m = PINN(box(R, P_LB, P_UB), HOLE, IC, LF, RT, UP, LW, DIST, lN, lS, lS, P_LB, P_UB, verbose=False)
    cand = box(R, P_LB, P_UB)
    cd = [torch.from_numpy(np.ascontiguousarray(cand[:, k], dtype=np.float32)).to(DEV) for k in range(3)]
    wq = m._score_weights(None)
    fc = m._frozen_at(cd)
    sr, sc = m._score_device(m._collo, m._frozen_collo, wq), m._score_device(cd, fc, wq)
    ci, ri = m.eng["uv"].select_k(sc, K, True).long(), m.eng["uv"].select_k(sr, K, False).long()
    pr, pc, _, _ = pair_replacements(ci, sc[ci], ri, sr[ri])
    scratch = m._frozen_collo.clone()

    def gather():
        for k in range(3):
            m._collo[k][pr] = cd[k][pc]
        scratch[..., pr] = fc[..., pc]

    rows = [("frozen D and P streams of the candidates (2 x net_streams 4 x 20)", timed(lambda: m._frozen_at(cd), a.reps)),
            ("score of the rows", timed(lambda: m._score_device(m._collo, m._frozen_collo, wq), a.reps)),
            ("score of the candidates", timed(lambda: m._score_device(cd, fc, wq), a.reps)),
            ("two selections", timed(lambda: (m.eng["uv"].select_k(sc, K, True), m.eng["uv"].select_k(sr, K, False)), a.reps)),
            ("pairing (two sorts of K, compare)", timed(lambda: pair_replacements(ci, sc[ci], ri, sr[ri]), a.reps)),
            (f"gathers: 3 coordinate columns + [2,5,5] frozen column of {int(pr.numel())} rows", timed(gather, a.reps))]
    m.refine_collocation(cand[:1000], 10)                       # (warm)
    info, ms = wall(lambda: m.refine_collocation(cand, K))
    lines += [f"PINN.refine_collocation, uv net 8 x 64, {R} rows, {R} candidates, n_replace = {K}: wall {ms:.1f} ms ({info['replaced']} rows replaced; "
              "includes the upload of the candidates and the host-copy update); its parts on the device:"] + fmt(rows)
    del m, fc, scratch, sr, sc
    torch.cuda.empty_cache()

    c = halfspace_case(n_collo=64, n_ic=64, n_top=64, n_src=(8, 8), seed=4, width=128, depth=10)
    m3 = NavierCauchy3D(box(R, N_LB, N_UB), c["SRC"], c["IC"], c["TOP"], l3, N_LB, N_UB, verbose=False)
    cand = box(R, N_LB, N_UB)
    cd = [torch.from_numpy(np.ascontiguousarray(cand[:, k], dtype=np.float32)).to(DEV) for k in range(4)]
    wq = m3._score_weights(None)
    rws = m3._rows(0, R)
    sr, sc = m3._score_device(rws, wq), m3._score_device(cd, wq)
    ci, ri = m3.engine.select_k(sc, K, True).long(), m3.engine.select_k(sr, K, False).long()
    pr, pc, _, _ = pair_replacements(ci, sc[ci], ri, sr[ri])
    scratch = [v.clone() for v in rws]

    def gather3():
        for k in range(4):
            scratch[k][pr] = cd[k][pc]

    rows = [("score of the rows", timed(lambda: m3._score_device(rws, wq), a.reps)),
            ("score of the candidates", timed(lambda: m3._score_device(cd, wq), a.reps)),
            ("two selections", timed(lambda: (m3.engine.select_k(sc, K, True), m3.engine.select_k(sr, K, False)), a.reps)),
            ("pairing (two sorts of K, compare)", timed(lambda: pair_replacements(ci, sc[ci], ri, sr[ri]), a.reps)),
            (f"gathers: 4 coordinate columns of {int(pr.numel())} rows", timed(gather3, a.reps))]
    m3.refine_collocation(cand[:1000], 10)
    info, ms = wall(lambda: m3.refine_collocation(cand, K))
    lines += [f"NavierCauchy3D.refine_collocation, net 10 x 128, {R} rows, {R} candidates, n_replace = {K}: wall {ms:.1f} ms ({info['replaced']} rows "
              "replaced; includes the upload of the candidates and the host-copy update); its parts on the device:"] + fmt(rows)
    lines.append(f"shader clock after the runs: {sclk()}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
