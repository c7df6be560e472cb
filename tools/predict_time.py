"""Times the predict heads on one GPU: wave_predict / plate_predict beside the route they replace on the device (fields /
net_streams, then the stack or composite of the model classes in torch), the fields call alone, one predict_frames of the
reference's post-processing grid and one validate.  Warm calls, HIP events around each call, median / min / max.
    python tools/predict_time.py [--points 1000000] [--reps 15] [--nets wave64,wave80,plate,class] [--out profiles/predict_head_calls.txt]
(PINN_HIP_LIB=<other build> --nets wave64,plate runs those blocks against a one-variant experiment build, e.g. one of tools/exp_build.sh
with Host::NB_PREDICT of pinn_host.hpp set to 2: the predict heads with two 16-point blocks per wave, the fields call's choice at width 64.)"""
import argparse
import os
import socket
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pinn_elastodynamics_amd import pointsets as ps                                        # noqa: E402
from pinn_elastodynamics_amd.elastic_wave import DeepHPM                                   # noqa: E402
from pinn_elastodynamics_amd.hip_engine import HipEngine                                   # noqa: E402
from tools.refine_family_time import P_LB, P_UB, cols, fmt, net                # noqa: E402
from tools.refine_time import sclk, timed                                                  # noqa: E402

DEV = torch.device("cuda:0")
W_LB, W_UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]


def wave_torch_route(eng, th, xs):
    """fields, then DeepHPM.predict's stack (elastic_wave.py) in torch on the device"""
    F = eng.fields(th, *xs, W_LB, W_UB, True)
    return torch.stack([F[0, 0], F[0, 1], F[0, 4], F[0, 5], F[0, 6], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]])


def plate_torch_route(eng, th, xs, fr):
    """net_streams of the uv net, then PINN._composite and predict's stack (plate_hole.py) in torch on the device"""
    N, D, P = eng.net_streams(th, *xs, P_LB, P_UB, False), fr[0], fr[1]
    F = torch.empty_like(N)
    F[0] = P[0] + D[0] * N[0]
    for k in (1, 2, 3):
        F[k] = P[k] + D[k] * N[0] + D[0] * N[k]
    F[4] = P[4] + D[4] * N[0] + 2.0 * D[3] * N[3] + D[0] * N[4]
    return torch.stack([F[0, 0], F[0, 1], F[0, 2], F[0, 3], F[0, 4], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]])


def block(title, new, old, alone, names, reps):
    a, b = new(), old()
    agree = float((a - b).abs().max() / b.abs().max())
    rows = [(names[0], timed(new, reps)), (names[1], timed(alone, reps)), (names[2], timed(old, reps))]
    return ([f"{title} (largest difference of the two routes' outputs / largest output: {agree:.1e})"] + fmt(rows)
            + [f"  predict / fields call alone = {rows[0][1][0] / rows[1][1][0]:.3f}   predict / replaced route = {rows[0][1][0] / rows[2][1][0]:.3f}"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--nets", default="wave64,wave80,plate,class")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, nets = a.points, a.nets.split(",")
    p = torch.cuda.get_device_properties(DEV)
    lines = [f"box {socket.gethostname()}: {p.name} ({getattr(p, 'gcnArchName', '?')}), {p.multi_processor_count} CUs",
             f"f16x3; median / min / max of {a.reps} warm calls, HIP events around each call [ms]; library {os.environ.get('PINN_HIP_LIB', 'in-tree')}"]
    for width in [w for w in (64, 80) if f"wave{w}" in nets]:
        lw = [3] + 8 * [width] + [7]
        eng, th, xs = HipEngine(lw, precision="f16x3", device=DEV, workspace_bytes=0), net(lw), cols(n, W_LB, W_UB, 1)
        out = torch.empty((8, n), dtype=torch.float32, device=DEV)
        lines += block(f"wave, net 8 x {width}, {n} points", lambda: eng.wave_predict(th, *xs, W_LB, W_UB, True, out=out), lambda: wave_torch_route(eng, th, xs),
                       lambda: eng.fields(th, *xs, W_LB, W_UB, True),
                       ("wave_predict (3 streams, 8 floats per point)", "fields (4 streams, 28 floats per point) alone", "fields + stack in torch (the route replaced)"), a.reps)
        del out, xs
    if "plate" in nets:
        lines += plate_block(n, a.reps)
    if "class" in nets:
        lines += class_block(a.reps)
    lines.append(f"shader clock after the runs: {sclk()}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def plate_block(n, reps):
    lN = [3] + 8 * [64] + [5]
    eng, th, xs = HipEngine(lN, precision="f16x3", device=DEV, workspace_bytes=0), net(lN), cols(n, P_LB, P_UB, 1)
    fr = (torch.randn((2, 5, 5, n), device=DEV) * torch.tensor([1.0, 2.0, 2.0, 0.2, 0.05], device=DEV)[None, :, None, None]).contiguous()
    out = torch.empty((8, n), dtype=torch.float32, device=DEV)
    return block(f"plate, uv net 8 x 64, {n} points, frozen streams resident", lambda: eng.plate_predict(th, *xs, P_LB, P_UB, False, fr, out=out),
                   lambda: plate_torch_route(eng, th, xs, fr), lambda: eng.net_streams(th, *xs, P_LB, P_UB, False),
                   ("plate_predict (3 streams, 8 floats per point)", "net_streams (5 streams, 25 floats per point) alone",
                    "net_streams + composite and stack in torch (the route replaced)"), reps)


def class_block(reps):
    # ---- the frame loop of the reference's post-processing (INF:752-766) and one validation, through the class
    c = ps.infinite_case(N_f=4000, N_ext=400, seed=3, width=64)
    m = DeepHPM(c["Collo"], c["SRC"], c["IC"], c["UP"], c["uv_layers"], c["lb"], c["ub"], verbose=False)
    g = np.linspace(0.0, 30.0, 201)
    gx, gy = (v.reshape(-1) for v in np.meshgrid(g, g))
    times = ps.frame_times(20.0)
    gxd, gyd, td = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) for v in (gx, gy, times))
    rows = [(f"predict_frames: 201 x 201 points x {times.size} frames, one predict call (tiling included)", timed(lambda: m.predict_frames(gxd, gyd, td), reps))]
    nv = 40401
    vx = cols(nv, W_LB, W_UB, 7)
    ref = {k: torch.randn(nv, device=DEV) for k in m.VALIDATE_FIELDS}
    rows.append((f"validate: {nv} points, 5 fields (reference resident; predict + error sums + download of 10 doubles)", timed(lambda: m.validate(*vx, ref), reps)))
    pred = m.predict_device(*vx)
    rr = torch.stack([ref[k] for k in m.VALIDATE_FIELDS]).contiguous()
    rows.append((f"field_error_sums alone: {nv} points, 5 rows", timed(lambda: m.engine.field_error_sums(pred, [0, 1, 2, 3, 4], rr), reps)))
    return ["DeepHPM, net 8 x 64:"] + fmt(rows)


if __name__ == "__main__":
    main()
