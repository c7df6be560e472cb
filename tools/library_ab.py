"""A / B of two builds of the library, bit for bit: every entry point that goes through a family's residual head (pinn_heads.hpp) or through a
summation scheme of pinn_reduce.hpp, on fixed inputs, with every output kept as raw bits.  What a refactor that must not change a result is held to.

    python tools/library_ab.py run LIB OUT.npz [--skip TEXT[,TEXT..]] [--only TEXT[,TEXT..]]      one fresh process per library
    python tools/library_ab.py compare A.npz B.npz                        one line per case, np.array_equal on the bits

LIB is a build of libpinn_hip.so (device tensors on cuda:0) or of the emulator library libpinn_emu.so (host arrays; chosen by the file's
name).  Inputs are those of the tests' case modules (tests/_refine_cases.py, _refine_family_cases.py, _material_family_cases.py,
_traction_cases.py): n in PRIMARY_N -- 1 and 33 leave padded lanes in a tile, 2100 in the minimum workspace makes the fp32 mode walk the
points in several passes --, one line per padded width plus one net of a compiled fused depth per family, the general material constants,
the case modules' weight tuples.  The wave family's step runs twice: pinn_wave2d_step with two value-only sets, and
pinn_wave2d_step_traction with a traction set (kind 2 of the fused one-stream head).  Every call runs in three forms where it has them: the default path, PINN_FLAG_TWO_KERNEL, PINN_PREC_FP32.
The reductions: the wave family also runs at n = 900 (REDUCE_N: the fused grid then has 1, 15 and 33 or 66 workgroups over the four n, so the
gradient column sum is entered with its remainder loop alone, with some waves in the unrolled loop, and with all of them; the loss walk with fewer
and with more than 32 waves), its step with and without the Adam epilogue, and once with a weight of 2100 (the NaN poison of the fused epilogues);
pinn_data_loss_grad_multi, pinn_stream_loss_grad_multi with three sets, pinn_adam_step; and the small kernels -- pinn_select_k,
pinn_refine_keys in both modes, pinn_binned_sums, pinn_field_error_sums, the three pinn_*_material_sums in PINN_PREC_FP32 with one pass -- at n = 1, 257
and the first size past the cap of tests/_grid_cap_cases.py, where a workgroup's range first exceeds one tile.
--skip leaves out the cases whose name contains one of the texts (an emulator run may leave the 10 x 128 net to the device), --only runs none
but those whose name contains one of its texts."""
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
REDUCE_N = (1, 33, 900, 2100)      # the wave family's sizes: tests/_refine_cases.PRIMARY_N and 900


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
        return self.put(np.full(count, np.nan if np.issubdtype(dtype, np.floating) else -1, dtype))

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
    def __init__(self, lib, mem, skip, only=()):
        self.lib, self.mem, self.skip, self.only, self.results = lib, mem, skip, only, {}

    def workspace(self, layers, n, form, mode):
        """the fp32 form in the minimum workspace (n = 2100 then takes several passes), the others in the workspace of the call's size"""
        lib = self.lib
        wsb = lib.min_workspace_bytes(layers, mode & 0xff) if form == "fp32" else lib.workspace_bytes(layers, max(n, 1 << 12), mode & 0xff)
        return self.mem.put(np.zeros((wsb + 3) // 4, np.uint32))[0], wsb

    def case(self, key, entry, form, fn):
        """fn() -> {name: handle}; keeps the bits under key/name"""
        if any(s in key for s in self.skip) or (self.only and not any(s in key for s in self.only)):
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
        for n in REDUCE_N:
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

                    def step(with_adam=True):
                        p, xs, ws, wsb = begin()
                        pp, hp = mem.put(flat)
                        st, hm, hv = adam(mem, flat.size)
                        st = st if with_adam else None
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
                                      ("step_no_adam", lambda: step(False)), ("step_traction", step_traction)):
                        R.case(f"{key}/{entry}", entry, form, fn)

                def traction():
                    ws, wsb = R.workspace(layers, n, form, mode)
                    (lo, hl), (gr, hg) = mem.out(8), mem.out(flat.size)
                    lib.wave2d_traction_loss_grad(mem.inp(flat), layers, *[mem.inp(XT[:, k]) for k in range(3)], n, RC.LB, RC.UB, True, mem.inp(aux),
                                                  TC.weights_for(n), lo, gr, False, mode, ws, wsb)
                    return {"loss": hl, "grad": hg}
                R.case(f"wave/{line}/{form}/n{n}/traction_loss_grad", "traction_loss_grad", form, traction)

                def data_multi():
                    ws, wsb = R.workspace(layers, n, form, mode)
                    (gr, hg), (s0, h0), (s1, h1) = mem.out(flat.size), mem.out(8), mem.out(8)
                    xt = [mem.inp(XT[:, k]) for k in range(3)]
                    tg = mem.inp(np.ascontiguousarray(aux[[2, 3, 2, 3, 2, 3, 2]]))
                    sets = [(*xt, n, 0, [1.0 / n, 2.0 / n, 0, 0, 0, 0, 0], s0), (*xt, n, tg, [0, 0, 0, 0, 0, 1.5 / n, 0.5 / n], s1)]
                    lib.data_loss_grad_multi(mem.inp(flat), layers, sets, RC.LB, RC.UB, True, gr, False, mode, ws, wsb)
                    return {"grad": hg, "set0": h0, "set1": h1}
                R.case(f"wave/{line}/{form}/n{n}/data_loss_grad_multi", "data_loss_grad_multi", form, data_multi)

    # a weight outside the fused format's range (|w| > 2047): the fused epilogues answer NaN as a whole, the other forms compute
    layers, n = [3] + 8 * [64] + [7], 33                          # (a compiled fused depth: the default form is the fused kernel)
    flat = RC.fresh_net(tuple(layers)).astype(np.float32)
    flat[3 * 64 + 64 + 3 * 64 + 5] = 2100.0                      # W1[3, 5]
    X = RC.points(n)
    for form, mode in forms("f16x3"):
        def poisoned(with_sets):
            ws, wsb = R.workspace(layers, n, form, mode)
            pp, hp = mem.put(flat)
            xs = [mem.inp(X[:, k]) for k in range(3)]
            (lo, hl), (gr, hg), (s0, h0) = mem.out(8), mem.out(flat.size), mem.out(8)
            tw = [w / n for w in RC.WEIGHTS]
            if with_sets:
                st, hm, hv = adam(mem, flat.size)
                lib.wave2d_step(pp, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, True, tw, lo, [(*xs, n, 0, [1.0 / n, 2.0 / n, 0, 0, 0, 0, 0], s0)], gr,
                                False, st, mode, ws, wsb)
                return {"loss": hl, "grad": hg, "set0": h0, "theta": hp, "m": hm, "v": hv}
            lib.wave2d_loss_grad(pp, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, True, tw, lo, gr, False, mode, ws, wsb)
            return {"loss": hl, "grad": hg}
        R.case(f"wave/fused8x64/{form}/n{n}/weight2100/loss_grad", "loss_grad", form, lambda: poisoned(False))
        R.case(f"wave/fused8x64/{form}/n{n}/weight2100/step", "step", form, lambda: poisoned(True))


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

    # pinn_stream_loss_grad_multi: three of the plate's pre-training sets (tests/_stream_sets.py), one with targets
    from tests import _stream_sets as SS
    # (4 x 20 and 4 x 64: the two layouts of fused_sets_kernel)
    for line, layers, sizes in [(f"fused4x{h}", [3] + 4 * [h] + [5], sz) for h in (20, 64) for sz in ((1, 33, 7), (900, 257, 2100))]:
        rng = np.random.default_rng(300 + sizes[0])
        flat = SS.fresh_net(layers, rng).astype(np.float32)
        sets = SS.make_sets(SS.PART_PATTERNS[:3], sizes, rng)
        for form, mode in forms("f16x3"):
            def stream_multi():
                ws, wsb = R.workspace(layers, sum(sizes), form, mode)
                (gr, hg), rows, outs = mem.out(flat.size), [], {}
                for k, (Xk, tg, w) in enumerate(sets):
                    lo, outs[f"set{k}"] = mem.out(8)
                    t32 = SS.device_targets(tg, w, False)
                    rows.append((*[mem.inp(Xk[:, j]) for j in range(3)], Xk.shape[0], 0 if t32 is None else mem.inp(t32), w.tolist(), lo))
                lib.stream_loss_grad_multi(mem.inp(flat), layers, rows, SS.LBP, SS.UBP, False, gr, False, mode, ws, wsb)
                return {"grad": hg, **outs}
            R.case(f"plate/{line}/{form}/n{'+'.join(map(str, sizes))}/stream_loss_grad_multi", "stream_loss_grad_multi", form, stream_multi)


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


def run_small(R, general):
    """pinn_adam_step and the kernels over contiguous per-workgroup ranges (reduce::split_ranges, range_of, records_sum)"""
    from tests import _causal_cases as CC
    from tests import _grid_cap_cases as GC
    from tests import _refine_cases as RC
    from tests import _sample_cases as SC
    lib, mem = R.lib, R.mem
    E, mu, rho = general
    on_device = mem.device is not None

    def adam_step():
        rng = np.random.default_rng(7)
        P = 1000
        hs = [mem.put(a.astype(np.float32)) for a in (rng.standard_normal(P), 0.01 * rng.standard_normal(P), 1e-4 * rng.random(P), rng.standard_normal(P))]
        lib.adam_step(hs[0][0], hs[1][0], hs[2][0], hs[3][0], P, 1e-3, 3)
        return {"theta": hs[0][1], "m": hs[1][1], "v": hs[2][1]}
    R.case("adam_step/n1000", "adam_step", "default", adam_step)

    def scratch(nbytes):
        return mem.put(np.zeros(nbytes // 4 + 1, np.uint32))[0], nbytes

    for n in (1, 257, GC.SELECT_N[0]):
        score = RC.select_data("ties", n)
        ks = sorted({1, max(n // 10, 1), max(n - 1, 1)}) if n < GC.SELECT_CAP else \
            sorted({GC.tie_k(score, True, n), GC.tie_k(score, False, n)} | ({n - 1} if on_device else set()))
        for k in ks:
            for largest in (True, False):
                def select():
                    idx, hi = mem.out(k, np.int32)
                    lib.select_k(mem.inp(score), n, k, largest, idx, *scratch(lib.select_workspace_bytes(n)))
                    return {"idx": hi}
                R.case(f"select_k/n{n}/k{k}/{'largest' if largest else 'smallest'}", "select_k", "default", select)
        pts, sc = SC.mask_points(3)[:n], SC.sample_scores(n)
        for kmode in ("mask", "sample"):
            def keys():
                key, hk = mem.out(n)
                lib.refine_keys(mem.inp(sc), n, mem.inp(pts[:, 0]), mem.inp(pts[:, 1]), None, [(*SC.DISC[0][:2], SC.DISC[1])], kmode, 0.5, 1.0, SC.KEY_SEED, SC.KEY_STREAM,
                                SC.KEY_FIRST, key, *scratch(lib.refine_keys_workspace_bytes(n)))
                return {"keys": hk}
            R.case(f"refine_keys/n{n}/{kmode}", "refine_keys", "default", keys)

    for n in (1, 257, GC.BINNED_N[0]):
        value, coord = CC.sums_case(n)
        for n_bins in GC.BINNED_BINS:
            def binned():
                so, hs = mem.out(2 * n_bins, np.float64)
                lib.binned_sums(mem.inp(value), mem.inp(coord), n, CC.LO, CC.HI, n_bins, so, *scratch(lib.binned_sums_workspace_bytes(n, n_bins)))
                return {"sums": hs}
            R.case(f"binned_sums/n{n}/bins{n_bins}", "binned_sums", "default", binned)

    for n in (1, 257, GC.FIELD_ERR_N[0]):
        for n_rows in (1, GC.MAX_ROWS):
            rows, pred, ref, _ = GC.error_case(n, n_rows)

            def err():
                so, hs = mem.out(2 * n_rows, np.float64)
                lib.field_error_sums(mem.inp(pred), GC.ERR_PRED_ROWS, rows, mem.inp(ref), n, so, *scratch(lib.field_error_workspace_bytes(n, n_rows)))
                return {"sums": hs}
            R.case(f"field_error_sums/n{n}/rows{n_rows}", "field_error_sums", "default", err)

    # PINN_PREC_FP32 material sums of the three families in ONE workspace pass of n points: material::fp32_partial_kernel<14 | 12> (the 3-D call: <12>
    # twice per pass) over ranges of more than one tile past its cap
    from tests import _refine_family_cases as FC
    for fam, din, nout, nsums in (("wave", 3, 7, 14), ("plate", 3, 5, 12), ("nc3d", 4, 12, 24)):
        layers = [din] + 2 * [16] + [nout]
        flat = FC.fresh_net(tuple(layers)).astype(np.float32)
        for n in (1, 257, GC.SELECT_N[0]):
            X = {"wave": RC.points, "plate": FC.plate_uniform, "nc3d": FC.nc3d_points}[fam](n)

            def sums():
                ws, wsb = scratch((GC.fp32_bytes_per_point(layers, GC.FP32_MAX_NS) * max(n, 256) + 255) // 256 * 256)      # room for all n points at once
                sb = lib.material_sums_workspace_bytes()
                (so, hs), sw = mem.out(nsums, np.float64), mem.put(np.zeros(sb // 8 + 1, np.float64))[0]
                p, xs, tail = mem.inp(flat), [mem.inp(X[:, k]) for k in range(din)], (so, PREC["fp32"], ws, wsb, sw, sb)
                if fam == "wave":
                    lib.wave2d_material_sums(p, layers, *xs, n, RC.LB, RC.UB, True, E, mu, rho, True, *tail)
                elif fam == "plate":
                    lib.plate2d_material_sums(p, layers, *xs, n, FC.PLATE_LB, FC.PLATE_UB, False, mem.inp(FC.plate_frozen(n)), E, mu, rho, *tail)
                else:
                    lib.nc3d_material_sums(p, layers, *xs, n, FC.NC3D_LB, FC.NC3D_UB, True, E, mu, rho, *tail)
                return {"sums": hs}
            R.case(f"material_one_pass/{fam}/w16/fp32/n{n}/material_sums", "material_sums", "fp32", sums)


def run(lib_path, out_path, skip, only=()):
    from tests._material_family_cases import GENERAL
    device = None
    if "emu" not in os.path.basename(lib_path):
        import torch
        device = torch.device("cuda:0")
    R = Runner(PinnLib(lib_path), Mem(device), skip, only)
    R.lib.set_fused(True)
    t0 = time.time()
    for fam in (run_wave, run_plate, run_nc3d, run_small):
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
        opts = {"--skip": [], "--only": []}
        for flag, texts in zip(sys.argv[4::2], sys.argv[5::2]):
            opts[flag] += texts.split(",")
        run(sys.argv[2], sys.argv[3], opts["--skip"], opts["--only"])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
