"""A / B of the residual heads, library against library: every entry point that goes through a family's residual head (pinn_heads.hpp), on
fixed inputs, with every output kept as raw bits.

    python tools/heads_ab.py run LIB OUT.npz [--skip TEXT[,TEXT..]]      one fresh process per library
    python tools/heads_ab.py compare A.npz B.npz                        one line per case, np.array_equal on the bits

LIB is a build of libpinn_hip.so (device tensors on cuda:0) or of the emulator library libpinn_emu.so (host arrays; chosen by the file's
name).  Inputs are those of the tests' case modules (tests/_refine_cases.py, _refine_family_cases.py, _material_family_cases.py,
_traction_cases.py): n in PRIMARY_N -- 1 and 33 leave padded lanes in a tile, 2100 in the minimum workspace makes the fp32 mode walk the
points in several passes --, one line per padded width plus one net of a compiled fused depth per family, the general material constants,
the case modules' weight tuples.  The wave family's step runs twice: pinn_wave2d_step with two value-only sets, and
pinn_wave2d_step_traction with a traction set (kind 2 of the fused one-stream head).  Every call runs in three forms where it has them: the default path, PINN_FLAG_TWO_KERNEL, PINN_PREC_FP32.
--skip leaves out the cases whose name contains one of the texts (an emulator run may leave the 10 x 128 net to the device)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pinn_elastodynamics_amd.capi import FLAG_TWO_KERNEL, PREC, PinnLib, PinnLibError  # noqa: E402

# entry points without a two-kernel form: forward only, they run chain_kernel whatever the flag says
FORWARD_ONLY = ("residual_score", "material_sums")


class Mem:
    """host arrays for the emulator library, device tensors for the HIP one"""

    def __init__(self, device):
        self.device, self.keep = device, []

    def put(self, a):
        """(pointer, handle) of a buffer holding the array `a`, 256-byte aligned"""
        a = np.ascontiguousarray(a)
        if self.device is None:
            raw = np.zeros(a.nbytes + 256, np.uint8)
            off = (-raw.ctypes.data) % 256
            h = raw[off:off + a.nbytes].view(a.dtype)
            h[:] = a.ravel()
            self.keep.append(raw)
            return h.ctypes.data, h
        import torch
        h = torch.from_numpy(a.ravel().copy()).to(self.device)
        self.keep.append(h)
        return h.data_ptr(), h

    def inp(self, a, dtype=np.float32):
        return self.put(np.asarray(a, dtype=dtype))[0]

    def out(self, count, dtype=np.float32):
        return self.put(np.full(count, np.nan, dtype))

    def bits(self, h):
        if self.device is not None:
            import torch
            torch.cuda.synchronize(self.device)
            h = h.cpu().numpy()
        return h.view(np.uint32 if h.dtype.itemsize == 4 else np.uint64).copy()


def forms(prec):
    if prec == "fp32":
        return (("fp32", PREC["fp32"]),)
    return (("default", PREC[prec]), ("two-kernel", PREC[prec] | FLAG_TWO_KERNEL), ("fp32", PREC["fp32"]))


class Runner:
    def __init__(self, lib, mem, skip):
        self.lib, self.mem, self.skip, self.results = lib, mem, skip, {}

    def workspace(self, layers, n, form, mode):
        """the fp32 form in the minimum workspace (n = 2100 then takes several passes), the others in the workspace of the call's size"""
        lib = self.lib
        wsb = lib.min_workspace_bytes(layers, mode & 0xff) if form == "fp32" else lib.workspace_bytes(layers, max(n, 1 << 12), mode & 0xff)
        return self.mem.put(np.zeros((wsb + 3) // 4, np.uint32))[0], wsb

    def case(self, key, entry, form, fn):
        """fn() -> {name: handle}; keeps the bits under key/name"""
        if any(s in key for s in self.skip):
            print(f"{key}: skipped on request")
            return
        if form == "two-kernel" and entry in FORWARD_ONLY:
            print(f"{key}: no such form (forward only: chain_kernel either way)")
            return
        self.lib.path_counts(reset=True)
        t0 = time.time()
        try:
            outs = fn()
        except PinnLibError as e:
            print(f"{key}: no such form ({e})")
            return
        bits = {k: self.mem.bits(h) for k, h in outs.items()}
        paths = ",".join(f"{k}:{v}" for k, v in self.lib.path_counts(reset=True).items() if v)
        for k, b in bits.items():
            self.results[f"{key}/{k}"] = b
        print(f"{key}: {paths}  {time.time() - t0:.1f} s", flush=True)
        self.mem.keep.clear()


def adam(mem, P):
    (pm, hm), (pv, hv) = mem.put(np.full(P, 0.01, np.float32)), mem.put(np.full(P, 0.02, np.float32))
    return (pm, pv, 1e-3, 0.9, 0.999, 1e-8, 3), hm, hv


def run_wave(R, general):
    from tests import _refine_cases as RC
    from tests import _traction_cases as TC
    lib, mem = R.lib, R.mem
    E, mu, rho = general
    for line, layers, prec in RC.PRIMARY_LINES + (("fused8x64", [3] + 8 * [64] + [7], "f16x3"),):
        flat = RC.fresh_net(tuple(layers)).astype(np.float32)
        for n in RC.PRIMARY_N:
            X = RC.points(n)
            XT, aux = TC.make_set(n, np.random.default_rng(100 + n))
            for form, mode in forms(prec):
                for ps in (True, False):
                    def begin():
                        ws, wsb = R.workspace(layers, n, form, mode)
                        return mem.inp(flat), [mem.inp(X[:, k]) for k in range(3)], ws, wsb
                    key = f"wave/{line}/{form}/n{n}/{'strain' if ps else 'stress'}"
                    tw = [w / n for w in RC.WEIGHTS]

                    def loss_grad():
                        p, xs, ws, wsb = begin()
                        (lo, hl), (gr, hg) = mem.out(8), mem.out(flat.size)
                        lib.wave2d_loss_grad(p, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, ps, tw, lo, gr, False, mode, ws, wsb)
                        return {"loss": hl, "grad": hg}

                    def score():
                        p, xs, ws, wsb = begin()
                        sc, hs = mem.out(n)
                        lib.wave2d_residual_score(p, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, ps, RC.WEIGHTS, sc, mode, ws, wsb)
                        return {"score": hs}

                    def sums():
                        p, xs, ws, wsb = begin()
                        sb = lib.material_sums_workspace_bytes()
                        (so, hs), sw = mem.out(14, np.float64), mem.put(np.zeros(sb // 8 + 1, np.float64))[0]
                        lib.wave2d_material_sums(p, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, ps, so, mode, ws, wsb, sw, sb)
                        return {"sums": hs}

                    def step():
                        p, xs, ws, wsb = begin()
                        pp, hp = mem.put(flat)
                        st, hm, hv = adam(mem, flat.size)
                        (lo, hl), (gr, hg), (s0, h0), (s1, h1) = mem.out(8), mem.out(flat.size), mem.out(8), mem.out(8)
                        xt = [mem.inp(XT[:, k]) for k in range(3)]
                        tg = mem.inp(np.ascontiguousarray(aux[[2, 3, 2, 3, 2, 3, 2]]))
                        sets = [(*xt, n, 0, [1.0 / n, 2.0 / n, 0, 0, 0, 0, 0], s0), (*xt, n, tg, [0, 0, 0, 0, 0, 1.5 / n, 0.5 / n], s1)]
                        lib.wave2d_step(pp, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, ps, tw, lo, sets, gr, False, st, mode, ws, wsb)
                        return {"loss": hl, "grad": hg, "set0": h0, "set1": h1, "theta": hp, "m": hm, "v": hv}

                    def step_traction():
                        # the step with one value-only set and the traction set (kind 2 of the one-stream head)
                        p, xs, ws, wsb = begin()
                        pp, hp = mem.put(flat)
                        st, hm, hv = adam(mem, flat.size)
                        (lo, hl), (gr, hg), (s0, h0), (tl, ht) = mem.out(8), mem.out(flat.size), mem.out(8), mem.out(8)
                        xt = [mem.inp(XT[:, k]) for k in range(3)]
                        sets = [(*xt, n, 0, [1.0 / n, 2.0 / n, 0, 0, 0, 0, 0], s0)]
                        lib.wave2d_step_traction(pp, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, ps, tw, lo, sets, *xt, n, mem.inp(aux),
                                                 TC.weights_for(n), tl, gr, False, st, mode, ws, wsb)
                        return {"loss": hl, "grad": hg, "set0": h0, "traction": ht, "theta": hp, "m": hm, "v": hv}

                    for entry, fn in (("loss_grad", loss_grad), ("residual_score", score), ("material_sums", sums), ("step", step),
                                      ("step_traction", step_traction)):
                        R.case(f"{key}/{entry}", entry, form, fn)

                def traction():
                    ws, wsb = R.workspace(layers, n, form, mode)
                    (lo, hl), (gr, hg) = mem.out(8), mem.out(flat.size)
                    lib.wave2d_traction_loss_grad(mem.inp(flat), layers, *[mem.inp(XT[:, k]) for k in range(3)], n, RC.LB, RC.UB, True, mem.inp(aux),
                                                  TC.weights_for(n), lo, gr, False, mode, ws, wsb)
                    return {"loss": hl, "grad": hg}
                R.case(f"wave/{line}/{form}/n{n}/traction_loss_grad", "traction_loss_grad", form, traction)


def run_plate(R, general):
    from tests import _refine_family_cases as FC
    lib, mem = R.lib, R.mem
    E, mu, rho = general
    LB, UB = FC.PLATE_LB, FC.PLATE_UB
    for line, layers, prec in FC.PLATE_LINES + (("fused8x64", [3] + 8 * [64] + [5], "f16x3"),):
        flat = FC.fresh_net(tuple(layers)).astype(np.float32)
        for n in FC.PRIMARY_N:
            X, frozen = FC.plate_uniform(n), FC.plate_frozen(n)
            th = 2.0 * np.pi * np.random.default_rng(200 + n).random(n)
            aux = np.concatenate([frozen[0, 0], frozen[1, 0], np.cos(th)[None], np.sin(th)[None]]).astype(np.float32)      # D0, P0, nx, ny
            tw, hw = [w / n for w in FC.PLATE_WEIGHTS], [1.0 / n, 2.5 / n]
            for form, mode in forms(prec):
                def begin():
                    ws, wsb = R.workspace(layers, n, form, mode)
                    return mem.inp(flat), [mem.inp(X[:, k]) for k in range(3)], ws, wsb
                key = f"plate/{line}/{form}/n{n}"

                def loss_grad():
                    p, xs, ws, wsb = begin()
                    (lo, hl), (gr, hg) = mem.out(8), mem.out(flat.size)
                    lib.plate2d_loss_grad(p, layers, *xs, n, LB, UB, False, mem.inp(frozen), E, mu, rho, tw, lo, gr, False, mode, ws, wsb)
                    return {"loss": hl, "grad": hg}

                def score():
                    p, xs, ws, wsb = begin()
                    sc, hs = mem.out(n)
                    lib.plate2d_residual_score(p, layers, *xs, n, LB, UB, False, mem.inp(frozen), E, mu, rho, FC.PLATE_WEIGHTS, sc, mode, ws, wsb)
                    return {"score": hs}

                def sums():
                    p, xs, ws, wsb = begin()
                    sb = lib.material_sums_workspace_bytes()
                    (so, hs), sw = mem.out(12, np.float64), mem.put(np.zeros(sb // 8 + 1, np.float64))[0]
                    lib.plate2d_material_sums(p, layers, *xs, n, LB, UB, False, mem.inp(frozen), E, mu, rho, so, mode, ws, wsb, sw, sb)
                    return {"sums": hs}

                def traction():
                    p, xs, ws, wsb = begin()
                    (lo, hl), (gr, hg) = mem.out(8), mem.out(flat.size)
                    lib.plate2d_traction_loss_grad(p, layers, *xs, n, LB, UB, False, mem.inp(aux), hw, lo, gr, False, mode, ws, wsb)
                    return {"loss": hl, "grad": hg}

                def step():
                    p, xs, ws, wsb = begin()
                    pp, hp = mem.put(flat)
                    st, hm, hv = adam(mem, flat.size)
                    (lo, hl), (gr, hg), (ho, hh) = mem.out(8), mem.out(flat.size), mem.out(8)
                    lib.plate2d_step(pp, layers, *xs, n, LB, UB, False, mem.inp(frozen), E, mu, rho, tw, lo, *xs, n, mem.inp(aux), hw, ho, gr, False, st,
                                     mode, ws, wsb)
                    return {"loss": hl, "grad": hg, "hole": hh, "theta": hp, "m": hm, "v": hv}

                for entry, fn in (("loss_grad", loss_grad), ("residual_score", score), ("material_sums", sums), ("traction_loss_grad", traction),
                                  ("step", step)):
                    R.case(f"{key}/{entry}", entry, form, fn)


def run_nc3d(R, general):
    from tests import _refine_family_cases as FC
    lib, mem = R.lib, R.mem
    E, mu, rho = general
    LB, UB = FC.NC3D_LB, FC.NC3D_UB
    for line, layers, prec in FC.NC3D_LINES + (("fused10x128", [4] + 10 * [128] + [12], "f16x3"),):
        flat = FC.fresh_net(tuple(layers)).astype(np.float32)
        for n in FC.PRIMARY_N:
            X = FC.nc3d_points(n)
            tw = [w / n for w in FC.NC3D_WEIGHTS]
            for form, mode in forms(prec):
                def begin():
                    ws, wsb = R.workspace(layers, n, form, mode)
                    return mem.inp(flat), [mem.inp(X[:, k]) for k in range(4)], ws, wsb
                key = f"nc3d/{line}/{form}/n{n}"

                def loss_grad():
                    p, xs, ws, wsb = begin()
                    (lo, hl), (gr, hg) = mem.out(16), mem.out(flat.size)
                    lib.nc3d_loss_grad(p, layers, *xs, n, LB, UB, True, E, mu, rho, tw, lo, gr, False, mode, ws, wsb)
                    return {"loss": hl, "grad": hg}

                def score():
                    p, xs, ws, wsb = begin()
                    sc, hs = mem.out(n)
                    lib.nc3d_residual_score(p, layers, *xs, n, LB, UB, True, E, mu, rho, FC.NC3D_WEIGHTS, sc, mode, ws, wsb)
                    return {"score": hs}

                def sums():
                    p, xs, ws, wsb = begin()
                    sb = lib.material_sums_workspace_bytes()
                    (so, hs), sw = mem.out(24, np.float64), mem.put(np.zeros(sb // 8 + 1, np.float64))[0]
                    lib.nc3d_material_sums(p, layers, *xs, n, LB, UB, True, E, mu, rho, so, mode, ws, wsb, sw, sb)
                    return {"sums": hs}

                for entry, fn in (("loss_grad", loss_grad), ("residual_score", score), ("material_sums", sums)):
                    R.case(f"{key}/{entry}", entry, form, fn)


def run(lib_path, out_path, skip):
    from tests._material_family_cases import GENERAL
    device = None
    if "emu" not in os.path.basename(lib_path):
        import torch
        device = torch.device("cuda:0")
    R = Runner(PinnLib(lib_path), Mem(device), skip)
    R.lib.set_fused(True)
    t0 = time.time()
    for fam in (run_wave, run_plate, run_nc3d):
        fam(R, GENERAL)
    np.savez_compressed(out_path, **R.results)
    print(f"{len(R.results)} arrays of {lib_path} in {time.time() - t0:.0f} s -> {out_path}")


def compare(path_a, path_b):
    A, B = np.load(path_a), np.load(path_b)
    cases = {}
    for k in sorted(set(A.files) | set(B.files)):
        case, name = k.rsplit("/", 1)
        same = k in A.files and k in B.files and A[k].dtype == B[k].dtype and np.array_equal(A[k], B[k])
        cases.setdefault(case, []).append((name, same))
    bad = 0
    for case, outs in cases.items():
        wrong = [nm for nm, same in outs if not same]
        bad += bool(wrong)
        print(f"{case}: " + ("bit-equal (" + ", ".join(nm for nm, _ in outs) + ")" if not wrong else "DIFFERENT in " + ", ".join(wrong)))
    print(f"{len(cases)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        skip = [s for a in sys.argv[4:] if not a.startswith("--") for s in a.split(",")]
        run(sys.argv[2], sys.argv[3], skip)
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
