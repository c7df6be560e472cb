"""The product of what ships: every line of pinn_elastodynamics_amd/csrc/pinn_variants.def (operand type x MFMAs per product x padded
width), plus PINN_PREC_FP32 as a pseudo-line, times every head pinn_path_for admits for it.  Plain helper module (not a conftest): the
emulator half (tests/test_emulated_kernels.py) and the GPU half (tests/test_gpu_variant_matrix.py) run the same rows through the same
checker, and the completeness test fails when a line, an admitted head or a path has no row.

Each row names a real hidden width and depth that land on the line, the head and the path pinn_path_for must name for it; the checker
asserts that path with pinn_debug_path_counts and compares every entry point of the head with the float64 oracle (loss sums, gradient,
fields / streams), with guard words behind every output, the accumulate / overwrite / empty-batch rules, the packed-weights flag and the
same call under PINN_FLAG_TWO_KERNEL."""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEF_PATH = os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc", "pinn_variants.def")
# the Makefile's pattern: sed -n 's/^PINN_VARIANT(\([A-Z0-9]*\), *\([0-9]*\), *\([0-9]*\))/.../p'
_LINE = re.compile(r"^PINN_VARIANT\(([A-Z0-9]*), *([0-9]*), *([0-9]*)\)", re.M)
PREC_OF = {("BF16", 1): "bf16", ("F16", 3): "f16x3", ("F16", 1): "f16", ("BF16", 3): "bf16x3"}
FP32_LINE = ("FP32", 0, 0)          # the pseudo-line of PINN_PREC_FP32 (no kernel family, every width)
WIDTHS = (32, 64, 96, 128, 160)
# real hidden widths that land on each padded width, the depths the fused kernel is compiled for (Host::fused_depth), one it is not
REAL_WIDTHS = {32: (20, 32), 64: (50, 64), 96: (70, 80), 128: (100,), 160: (140,)}
FUSED_DEPTHS = {32: (4, 8), 64: (4, 8), 96: (8,), 128: (8,), 160: (6,)}
OFF_DEPTH = {32: 3, 64: 5, 96: 5, 128: 3, 160: 3}
HEADS = ("wave", "data", "plate", "streams", "nc3d", "nc3d_data")
NOUT = {"wave": 7, "data": 7, "plate": 5, "streams": 5, "nc3d": 12, "nc3d_data": 12}
PATHS = ("fused-registers", "fused-lds", "two-kernel", "fp32")
# relative L2 bars of loss sums / gradient / fields on fresh weights: TOL of tests/test_gpu_parity.py, fp32 from tests/test_gpu_paths.py
BAR = {"f16x3": 2e-5, "bf16x3": 2e-4, "f16": 5e-3, "bf16": 3e-2, "fp32": 1e-4}
# include/pinn_hip.h (PINN_PREC_F16X3 (2), PINN_PREC_BF16X3): the weight gradient of the narrow (padded width <= 64) fused kernels
# multiplies 16-bit high parts of the layer states -- a rounding noise c / sqrt(points) relative to the gradient.  Measured on an MI355X
# at fresh weights (n = 64 / 1024 / 16384, four draws each; mean and worst c): four-stream wave head 3e-4 / 3.8e-4 (bf16x3 2.5e-3 /
# 3.5e-3), one-stream value heads 7e-4 / 9e-4 (5.5e-3 / 8e-3), five-stream plate head 1.1e-3 / 2.6e-3 (9e-3 / 2.2e-2).  The bars hold
# about three times the mean (the wave head's f16x3 bar is tests/test_gpu_paths.py's); tools/narrow_noise_study.py repeats the measurement.
NARROW_NOISE = {("f16x3", "wave"): 6e-4, ("f16x3", "data"): 2.5e-3, ("f16x3", "plate"): 5e-3,
                ("bf16x3", "wave"): 8e-3, ("bf16x3", "data"): 2e-2, ("bf16x3", "plate"): 4e-2}
SENTINEL = np.uint32(0x7FA5A5A5)    # a NaN payload no arithmetic produces: the guard words behind every output
GUARD = 64                          # 256 bytes of guard words


def variant_lines(path=DEF_PATH):
    with open(path) as f:
        return [(op, int(split), int(width)) for op, split, width in _LINE.findall(f.read())]


def prec_of(line):
    return "fp32" if line == FP32_LINE else PREC_OF.get(line[:2])


@dataclass(frozen=True)
class Row:
    prec: str
    hidden: int
    depth: int
    head: str
    path: str

    @property
    def din(self):
        return 4 if self.head.startswith("nc3d") else 3

    @property
    def layers(self):
        return [self.din] + self.depth * [self.hidden] + [NOUT[self.head]]

    @property
    def width(self):
        return next(w for w in WIDTHS if self.hidden <= w)

    @property
    def line(self):
        if self.prec == "fp32":
            return FP32_LINE
        op, split = next(k for k, v in PREC_OF.items() if v == self.prec)
        return (op, split, self.width)

    @property
    def tiles(self):
        """16-point tiles per workgroup step of the fused layout (pinn_fused.hpp: 4 for the register layouts, 2 for the LDS-operand ones)"""
        return 2 if self.width > 64 else 4

    @property
    def sizes(self):
        t = 16 * self.tiles
        return (1, 15, 16, 17, t - 1, t + 1)

    def __str__(self):
        return f"{self.prec}-{self.depth}x{self.hidden}-{self.head}-{self.path}"


def R(prec, hidden, depth, heads, path):
    return [Row(prec, hidden, depth, h, path) for h in heads.split()]


# ---- the rows.  One per (line, admitted head) on the path the line's fused depth takes, a two-kernel row per line at a depth the fused
# kernel is not compiled for, every fp32 head.  Kept small (one real width per padded width, the shallowest compiled depth): the
# emulator runs each row at six sizes.
ROWS = (
    R("bf16", 20, 4, "wave data", "fused-registers") + R("bf16", 20, 3, "wave", "two-kernel")
    + R("bf16", 50, 4, "wave data", "fused-registers") + R("bf16", 50, 5, "data", "two-kernel")
    + R("bf16", 70, 8, "wave data", "two-kernel")               # padded widths 96 / 128 / 160 in bf16: no fused instantiation
    + R("bf16", 100, 2, "wave data", "two-kernel")
    + R("bf16", 140, 2, "wave data", "two-kernel")
    + R("f16x3", 20, 4, "wave data plate", "fused-registers") + R("f16x3", 20, 2, "streams nc3d nc3d_data", "two-kernel")
    + R("f16x3", 50, 4, "wave data plate", "fused-registers") + R("f16x3", 50, 5, "plate", "two-kernel")
    + R("f16x3", 50, 2, "streams nc3d nc3d_data", "two-kernel")
    + R("f16x3", 70, 8, "wave data plate", "fused-lds") + R("f16x3", 70, 2, "streams nc3d nc3d_data", "two-kernel")
    + R("f16x3", 100, 8, "wave data", "fused-lds") + R("f16x3", 100, 2, "plate streams", "two-kernel")
    + R("f16x3", 100, 10, "nc3d nc3d_data", "fused-lds")
    + R("f16x3", 140, 6, "wave data", "fused-lds") + R("f16x3", 140, 2, "plate streams nc3d nc3d_data", "two-kernel")
    + R("f16", 50, 4, "wave data", "fused-registers") + R("f16", 50, 3, "wave", "two-kernel")
    + R("bf16x3", 50, 4, "wave data plate", "fused-registers") + R("bf16x3", 50, 3, "data", "two-kernel")
    + R("bf16x3", 50, 2, "streams nc3d nc3d_data", "two-kernel")
    + R("fp32", 20, 3, "wave data plate streams nc3d nc3d_data", "fp32")
)


def generated_cases(lines):
    """(line, head, layers) over every line x real width x (compiled depths, one other depth) x head: what the completeness test asks
    pinn_path_for about (a line whose width has no real widths here yields a None layer list, which the test reports)"""
    for line in list(lines) + [FP32_LINE]:
        widths = WIDTHS if line == FP32_LINE else (line[2],)
        for w in widths:
            if w not in REAL_WIDTHS:
                yield line, None, None
                continue
            for h in REAL_WIDTHS[w]:
                for head in HEADS:
                    din = 4 if head.startswith("nc3d") else 3
                    depths = FUSED_DEPTHS[w] + (OFF_DEPTH[w],) + ((10,) if din == 4 and w == 128 else ())
                    for d in depths:
                        yield line, head, [din] + d * [h] + [NOUT[head]]


# ---- memory: host arrays for the emulator, device tensors on the GPU; every output carries GUARD sentinel words behind it -------------
class Mem:
    def __init__(self, device=None):
        self.device = device
        self.keep = []

    def _u32(self, host):
        """a 256-byte aligned buffer holding the uint32 array `host`; returns (pointer, handle)"""
        if self.device is None:
            raw = np.zeros(host.size * 4 + 256, np.uint8)
            off = (-raw.ctypes.data) % 256
            a = raw[off:off + host.size * 4].view(np.uint32)
            a[:] = host
            self.keep.append(raw)
            return a.ctypes.data, a
        import torch
        t = torch.from_numpy(host.view(np.int32).copy()).to(self.device)
        self.keep.append(t)
        return t.data_ptr(), t

    def inp(self, a):
        """read-only float32 input (0 for an empty array, as a caller passes NULL)"""
        a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        if a.size == 0:
            return 0
        return self._u32(a.view(np.uint32))[0]

    def out(self, count, fill=np.nan):
        return Out(self, count, fill)

    def ws(self, nbytes):
        return self._u32(np.zeros((nbytes + 3) // 4, np.uint32))[0]

    def read(self, h):
        if self.device is None:
            return h.copy()
        import torch
        torch.cuda.synchronize(self.device)
        return h.cpu().numpy().view(np.uint32)


class Out:
    def __init__(self, mem, count, fill):
        self.mem, self.count = mem, count
        host = np.full(count + GUARD, SENTINEL, np.uint32)
        host[:count] = np.array([fill] * count, np.float32).view(np.uint32)
        self.ptr, self.h = mem._u32(host)

    def bits(self):
        return self.mem.read(self.h)

    def values(self):
        b = self.bits()
        assert np.all(b[self.count:] == SENTINEL), f"write past the end of a {self.count}-float output: guard words " \
            f"{np.flatnonzero(b[self.count:] != SENTINEL)[:8].tolist()} changed"
        return b[:self.count].view(np.float32).astype(np.float64)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a))


def grad_bar(row, n, path, head=None):
    bar = BAR[row.prec]
    key = (row.prec, head or row.head)
    if path == "fused-registers" and key in NARROW_NOISE:
        bar = max(bar, NARROW_NOISE[key] / np.sqrt(max(n, 1)))
    return bar


# ---- the per-head problems: inputs, float64 oracle, and the library calls ---------------------------------------------------------------
LB, UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
LBP, UBP = [0.0, 0.0, 0.0], [0.5, 0.5, 10.0]
LB3, UB3 = [0.0, 0.0, -20.0, 0.0], [30.0, 30.0, 0.0, 15.0]
LD = [3, 10, 10, 5]         # the plate's frozen distance / particular nets


def _net(layers, rng, bias=0.2):
    Ws, bs = po.xavier_init(layers, rng)
    return po.pack_params(Ws, [bias * rng.standard_normal(b.shape) for b in bs])


class Problem:
    """one row at one size: points, parameters and oracle values; call(entry, mode, accumulate, grad_fill) runs an entry point"""

    def __init__(self, lib, mem, row, n, seed=0, ws_bytes=None):
        self.lib, self.mem, self.row, self.n = lib, mem, row, n
        rng = np.random.default_rng(seed + 1000 * n)
        L = row.layers
        self.flat = _net(L, rng)
        self.P = self.flat.size
        self.params = mem.inp(self.flat)
        m = max(n, 1)
        head = row.head
        if head in ("wave", "data"):
            X = po.collocation_points(n, LB, UB, rng) if n else np.zeros((0, 3))
        elif head in ("plate", "streams"):
            X = np.stack([rng.random(n) * 0.5, rng.random(n) * 0.5, rng.random(n) * 10], 1)
        else:
            X = n3.halfspace_points(n, LB3, UB3, rng) if n else np.zeros((0, 4))
        self.X = X
        self.xs = [mem.inp(X[:, k]) for k in range(X.shape[1])]
        self.ref = {}
        if head in ("wave", "data"):
            self.tw = np.array([1, 2, 3, 1, 0.5, 1, 2.0]) / m
            self.tgt = rng.standard_normal((n, 7))
            self.tg = mem.inp(self.tgt.T)
            self.ow = np.array([1, 1, 0, 0, 0, 2, 0.5]) / m             # with targets
            self.ow0 = np.array([1, 1, 1, 1, 0, 0, 0.0]) / m            # without (the side set of the step call)
            if n:
                self.ref["data"] = po.data_loss_grad(self.flat, L, *X.T, LB, UB, True, self.tgt, self.ow)[:2]
                self.ref["data0"] = po.data_loss_grad(self.flat, L, *X.T, LB, UB, True, None, self.ow0)[:2]
                if head == "wave":
                    self.ref["loss"] = po.wave2d_loss_grad(self.flat, L, *X.T, LB, UB, True, term_weights=self.tw)[:2]
                    f = po.wave2d_fields(self.flat, L, *X.T, LB, UB, True)
                    self.ref["fields"] = np.concatenate([f["Y"].T] + [d.T for d in f["dY"]]).ravel()
                else:
                    self.ref["loss"] = self.ref["data"]
        if head == "plate":
            fD, fP = _net(LD, rng), _net(LD, rng)
            self.tw = np.array([10, 7, 13, 9, 11.0]) / m
            th = rng.random(n) * np.pi / 2
            H = np.stack([0.1 * np.cos(th), 0.1 * np.sin(th), rng.random(n) * 10], 1)
            self.hs = [mem.inp(H[:, k]) for k in range(3)]
            self.hw = [10.0 / m] * 2
            if n:
                D, Pp = pl.net_streams(fD, LD, *X.T), pl.net_streams(fP, LD, *X.T)
                ss, g, _ = pl.plate_loss_grad(self.flat, L, *X.T, D, Pp, term_weights=self.tw)
                self.ref["loss"] = (ss, g)
                DH, PH = pl.net_streams(fD, LD, *H.T)[0], pl.net_streams(fP, LD, *H.T)[0]
                self.ref["traction"] = pl.traction_loss_grad(self.flat, L, *H.T, DH, PH, weight=10.0 / m)
                frozen, aux = np.stack([D, Pp]), np.concatenate([DH, PH, (-H[:, 0] / 0.1)[None], (-H[:, 1] / 0.1)[None]])
            else:
                frozen, aux = np.zeros(0), np.zeros(0)
            self.frozen, self.aux = mem.inp(frozen), mem.inp(aux)
        if head == "streams":
            self.tgt = rng.standard_normal((5, 5, n))
            self.w = np.zeros((5, 5))
            self.w[0, :] = 1000.0 / m
            self.w[3, 0] = self.w[3, 1] = 500.0 / m
            self.tg = mem.inp(self.tgt)
            if n:
                s3, g3 = pl.stream_loss_grad(self.flat, L, *X.T, self.tgt, self.w)
                self.ref["loss"] = (((self.w / self.w.max()) * s3).sum(0), g3)
                self.ref["streams"] = pl.net_streams(self.flat, L, *X.T).ravel()
        if head in ("nc3d", "nc3d_data"):
            self.tw = (0.5 + rng.random(12)) / m
            self.tgt = rng.standard_normal((n, 12))
            self.ow = np.array([1, 1, 1, 0.5, 0.5, 0.5, 0, 0, 2, 0, 2, 2.0]) / m
            self.tg = mem.inp(self.tgt.T)
            if n:
                ssd, gd, _ = n3.nc3d_data_loss_grad(self.flat, L, *X.T, LB3, UB3, True, self.tgt, self.ow)
                ss, g, _ = n3.nc3d_loss_grad(self.flat, L, *X.T, LB3, UB3, True, term_weights=self.tw)
                self.ref["loss"] = (ss, g) if head == "nc3d" else (ssd, gd)
                self.ref["data"] = (ssd, gd)
                f = n3.nc3d_fields(self.flat, L, *X.T, LB3, UB3, True)
                self.ref["fields"] = np.concatenate([f["Y"].T[None]] + [d.T[None] for d in f["dY"]]).ravel()
        self.wsb = max(lib.workspace_bytes(L, m, row.prec), lib.min_workspace_bytes(L, row.prec))
        if head == "plate":          # (the step call holds the collocation set and the hole set)
            self.wsb = max(self.wsb, lib.workspace_bytes(L, 2 * m, row.prec))
        if ws_bytes is not None:
            self.wsb = ws_bytes
        self.ws = mem.ws(self.wsb)

    def call(self, entry, mode, accumulate=False, grad_fill=np.nan, params=None, loss_fill=np.nan):
        """run one entry point; returns (loss_sums, gradient) as float64 (the guard words checked), or the fields / streams"""
        lib, mem, row, n, L = self.lib, self.mem, self.row, self.n, self.row.layers
        p = self.params if params is None else params
        loss = mem.out(2 if entry == "traction" else NOUT[self.row.head], loss_fill)
        grad = mem.out(self.P, grad_fill)
        ws = (self.ws, self.wsb)
        x = self.xs
        if entry == "wave":
            lib.wave2d_loss_grad(p, L, *x, n, LB, UB, True, 2.5, 0.25, 1.0, True, self.tw, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "data":
            lib.data_loss_grad(p, L, *x, n, LB, UB, True, self.tg, self.ow, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "data0":
            lib.data_loss_grad(p, L, *x, n, LB, UB, True, 0, self.ow0, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "plate":
            lib.plate2d_loss_grad(p, L, *x, n, LBP, UBP, False, self.frozen, 20.0, 0.25, 1.0, self.tw, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "traction":
            lib.plate2d_traction_loss_grad(p, L, *self.hs, n, LBP, UBP, False, self.aux, self.hw, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "streams":
            lib.stream_loss_grad(p, L, *x, n, LBP, UBP, False, self.tg, self.w, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "nc3d":
            lib.nc3d_loss_grad(p, L, *x, n, LB3, UB3, True, 2.5, 0.25, 1.0, self.tw, loss.ptr, grad.ptr, accumulate, mode, *ws)
        elif entry == "nc3d_data":
            lib.nc3d_data_loss_grad(p, L, *x, n, LB3, UB3, True, self.tg, self.ow, loss.ptr, grad.ptr, accumulate, mode, *ws)
        else:
            raise ValueError(entry)
        return loss.values(), grad.values()

    def fields(self, mode):
        lib, mem, n, L = self.lib, self.mem, self.n, self.row.layers
        if self.row.head == "wave":
            out = mem.out(28 * n)
            lib.wave2d_fields(self.params, L, *self.xs, n, LB, UB, True, out.ptr, mode, self.ws, self.wsb)
        elif self.row.head == "streams":
            out = mem.out(25 * n)
            lib.net_streams(self.params, L, *self.xs, n, LBP, UBP, False, out.ptr, mode, self.ws, self.wsb)
        else:
            out = mem.out(60 * n)
            lib.nc3d_fields(self.params, L, *self.xs, n, LB3, UB3, True, out.ptr, mode, self.ws, self.wsb)
        return out.values()

    def multi(self, mode, packed=False):
        """pinn_data_loss_grad_multi: the targets set, an empty set, the target-free set"""
        lib, mem, n, L = self.lib, self.mem, self.n, self.row.layers
        outs = [mem.out(7) for _ in range(3)]
        sets = [(*self.xs, n, self.tg, self.ow, outs[0].ptr), (0, 0, 0, 0, 0, self.ow0, outs[1].ptr), (*self.xs, n, 0, self.ow0, outs[2].ptr)]
        grad = mem.out(self.P)
        lib.data_loss_grad_multi(self.params, L, sets, LB, UB, True, grad.ptr, False, mode | (0x100 if packed else 0), self.ws, self.wsb)
        return [o.values() for o in outs], grad.values()

    def wave_step(self, mode):
        """pinn_wave2d_step with one side set (the target-free value head on the same points) and Adam from zero moments"""
        lib, mem, n, L = self.lib, self.mem, self.n, self.row.layers
        params = mem._u32(self.flat.astype(np.float32).view(np.uint32).copy())
        pm, pv = mem.out(self.P, 0.0), mem.out(self.P, 0.0)
        loss, sloss, grad = mem.out(7), mem.out(7), mem.out(self.P)
        sets = [(*self.xs, n, 0, self.ow0, sloss.ptr)]
        lr = 1e-3
        lib.wave2d_step(params[0], L, *self.xs, n, LB, UB, True, 2.5, 0.25, 1.0, True, self.tw, loss.ptr, sets, grad.ptr, False,
                        (pm.ptr, pv.ptr, lr, 0.9, 0.999, 1e-8, 1), mode, self.ws, self.wsb)
        new = mem.read(params[1]).view(np.float32).astype(np.float64)
        return loss.values(), sloss.values(), grad.values(), new, pm.values(), pv.values(), lr

    def plate_step(self, mode):
        lib, mem, n, L = self.lib, self.mem, self.n, self.row.layers
        loss, hloss, grad = mem.out(5), mem.out(2), mem.out(self.P)
        lib.plate2d_step(self.params, L, *self.xs, n, LBP, UBP, False, self.frozen, 20.0, 0.25, 1.0, self.tw, loss.ptr, *self.hs, n, self.aux,
                         self.hw, hloss.ptr, grad.ptr, False, None, mode, self.ws, self.wsb)
        return loss.values(), hloss.values(), grad.values()


def mode_word(prec, two_kernel=False, packed=False):
    from pinn_elastodynamics_amd.capi import FLAG_TWO_KERNEL, FLAG_WEIGHTS_PACKED, PREC
    return PREC[prec] | (FLAG_TWO_KERNEL if two_kernel else 0) | (FLAG_WEIGHTS_PACKED if packed else 0)


def counted(lib, path, fn, calls=1):
    lib.path_counts(reset=True)
    out = fn()
    pc = lib.path_counts(reset=True)
    assert pc[path] == calls and sum(pc.values()) == calls, (path, pc)
    return out


def check_row(lib, mem, row, n, full=True, seed=0, two_kernel=True):
    """Every check of one row at one size (see the module docstring).  `full` = False: the head's primary entry point only (with its
    path, guard words and the two-kernel comparison) -- the GPU's full-grid sizes, where the oracle is the expensive part."""
    path = lib.path_for(row.layers, row.prec, row.head)
    assert path == row.path, (str(row), path)
    pb = Problem(lib, mem, row, n, seed)
    prec, head = row.prec, row.head
    m0 = mode_word(prec)
    entry = head           # (each head's loss + gradient entry point has the head's name in Problem.call)
    bar, gbar, dbar = BAR[prec], grad_bar(row, n, path), grad_bar(row, n, path, "data")
    tag = f"{row} n={n}"
    loss, grad = counted(lib, path, lambda: pb.call(entry, m0))
    ss, g = pb.ref["loss"]
    assert rel(loss, ss) < bar, (tag, "loss", rel(loss, ss), bar)
    assert rel(grad, g) < gbar, (tag, "grad", rel(grad, g), gbar)
    if path.startswith("fused") and (two_kernel or full):           # the same call off the fused kernel
        loss2, grad2 = counted(lib, "two-kernel", lambda: pb.call(entry, mode_word(prec, two_kernel=True)))
        assert rel(loss2, ss) < bar and rel(grad2, g) < BAR[prec], (tag, "two-kernel", rel(loss2, ss), rel(grad2, g))
    if not full:
        return rel(grad, g)
    # accumulate onto a finite sentinel; the packed flag on the same workspace gives the same bits
    sentinel = 0.375
    _, grada = pb.call(entry, m0, accumulate=True, grad_fill=sentinel)
    assert rel(grada - sentinel, g) < gbar, (tag, "accumulate is not sentinel + gradient", rel(grada - sentinel, g))
    loss_p, grad_p = pb.call(entry, mode_word(prec, packed=True))
    assert np.array_equal(loss_p, loss) and np.array_equal(grad_p, grad), (tag, "packed flag changed the bits")
    # per head: the other entry points
    if head == "wave":
        f = pb.fields(m0)
        assert rel(f, pb.ref["fields"]) < bar, (tag, "fields", rel(f, pb.ref["fields"]))
        # wave -> data_multi on the same workspace, as the model class's step does: packed weights are valid for the value head
        pb.call(entry, m0)
        so, sg = pb.multi(m0)
        pb.call(entry, m0)
        sp, gp = pb.multi(m0, packed=True)
        assert all(np.array_equal(a, b) for a, b in zip(so, sp)) and np.array_equal(sg, gp), (tag, "wave -> multi packed")
        sl, ssl, sg, new, mm, vv, lr = pb.wave_step(m0)
        ssd, gd = pb.ref["data0"]
        assert rel(sl, ss) < bar and rel(ssl, ssd) < bar, (tag, "step loss sums")
        assert rel(sg, g + gd) < max(gbar, dbar), (tag, "step gradient", rel(sg, g + gd))
        th, m_, v_ = po.adam_tf1_step(pb.flat.astype(np.float32).astype(np.float64), sg, np.zeros(pb.P), np.zeros(pb.P), 1, lr)
        assert rel(new, th) < 1e-6 and rel(mm, m_) < 1e-6 and rel(vv, v_) < 1e-4, (tag, "step Adam", rel(new, th), rel(mm, m_), rel(vv, v_))
    elif head == "data":
        l0, g0 = pb.call("data0", m0)
        ss0, gg0 = pb.ref["data0"]
        assert rel(l0, ss0) < bar and rel(g0, gg0) < gbar, (tag, "data without targets", rel(l0, ss0), rel(g0, gg0))
        so, sg = pb.multi(m0)
        assert rel(so[0], ss) < bar and np.all(so[1] == 0) and rel(so[2], ss0) < bar, (tag, "multi sums")
        assert rel(sg, g + gg0) < dbar, (tag, "multi gradient", rel(sg, g + gg0))
    elif head == "plate":
        lt, gt = pb.call("traction", m0)
        sst, ggt = pb.ref["traction"]
        assert rel(lt, sst) < bar and rel(gt, ggt) < dbar, (tag, "traction", rel(lt, sst), rel(gt, ggt))
        # plate -> traction with packed weights, as the model class's step does
        lt2, gt2 = pb.call("traction", mode_word(prec, packed=True))
        assert np.array_equal(lt2, lt) and np.array_equal(gt2, gt), (tag, "plate -> traction packed")
        sl, hl, sg = pb.plate_step(m0)        # (fp32 and the two-kernel layouts: the two calls one after the other inside)
        assert rel(sl, ss) < bar and rel(hl, sst) < bar and rel(sg, g + ggt) < gbar, (tag, "plate step", rel(sg, g + ggt))
    elif head == "streams":
        s = pb.fields(m0)
        assert rel(s, pb.ref["streams"]) < bar, (tag, "net_streams", rel(s, pb.ref["streams"]))
    elif head in ("nc3d", "nc3d_data"):
        f = pb.fields(m0)
        assert rel(f, pb.ref["fields"]) < bar, (tag, "nc3d_fields", rel(f, pb.ref["fields"]))
        if head == "nc3d":         # 3-D collocation -> 3-D data with packed weights, as the model class's step does
            ld, gd = pb.call("nc3d_data", mode_word(prec, packed=True))
            ssd, gdd = pb.ref["data"]
            assert rel(ld, ssd) < bar and rel(gd, gdd) < BAR[prec], (tag, "nc3d -> data packed", rel(gd, gdd))
            ld0, gd0 = pb.call("nc3d_data", m0)
            assert np.array_equal(ld, ld0) and np.array_equal(gd, gd0), (tag, "nc3d -> data packed bits")


def check_empty(lib, mem, row):
    """n = 0: zero sums; the gradient zeroed (overwrite) or untouched (accumulate); nothing written past the outputs"""
    pb = Problem(lib, mem, row, 0)
    for acc in (False, True):
        loss, grad = pb.call(row.head, mode_word(row.prec), accumulate=acc, grad_fill=3.0, loss_fill=np.nan)
        assert np.all(loss == 0) and np.all(grad == (3.0 if acc else 0.0)), (str(row), acc)


def check_walk(lib, mem, row, n, grid_cap=0, min_ws=False):
    """the primary entry point with several workgroup steps per workgroup (a fused grid capped at `grid_cap` workgroups) or with
    pinn_min_workspace_bytes (smaller than the n-point workspace: the call walks the points in chunks, or leaves the fused kernel when the
    workspace holds too few scratch images -- pinn_path_for says which, the counters confirm it), against the oracle; guard words as
    everywhere"""
    ws = None
    path = row.path
    if min_ws:
        ws = lib.min_workspace_bytes(row.layers, row.prec)
        assert ws < lib.workspace_bytes(row.layers, n, row.prec), (str(row), n, "the minimum workspace holds all points: nothing to walk")
        path = lib.path_for(row.layers, row.prec, row.head, ws)
    pb = Problem(lib, mem, row, n, seed=7, ws_bytes=ws)
    old = lib.lib.pinn_debug_set_fused_grid_cap(grid_cap)
    try:
        loss, grad = counted(lib, path, lambda: pb.call(row.head, mode_word(row.prec)))
    finally:
        lib.lib.pinn_debug_set_fused_grid_cap(old)
    ss, g = pb.ref["loss"]
    assert rel(loss, ss) < BAR[row.prec] and rel(grad, g) < grad_bar(row, n, path), (str(row), n, grid_cap, min_ws, rel(loss, ss), rel(grad, g))
