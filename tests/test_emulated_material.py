"""CPU tests of pinn_wave2d_material_sums: the kernel sources compiled for x86 against the SIMT emulator, on host arrays framed by guard words that
are checked after every call (as in test_emulated_refine.py).  The 14 sums are compared with the formulas in float64 on the library's own fields call
(head rounding only), with the loss call's sums of squares, and with the float64 oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _material_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, stdout=subprocess.DEVNULL)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


class Guarded:
    """nbytes of payload at a 256-byte aligned address (+ `skew` bytes), guard words in front and behind"""

    def __init__(self, nbytes, skew=0, fill=0xA5):
        self.raw = np.full(nbytes + 2 * GUARD + 512 + skew, 0xA5, dtype=np.uint8)
        base = self.raw.ctypes.data
        self.off = (-(base + GUARD) % 256) + GUARD + skew
        self.nbytes = nbytes
        self.ptr = base + self.off
        self.raw[self.off:self.off + nbytes] = fill

    def view(self, dtype):
        return self.raw[self.off:self.off + self.nbytes].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:self.off] == 0xA5).all() and (self.raw[self.off + self.nbytes:] == 0xA5).all())


def put(a):
    g = Guarded(a.nbytes)
    g.view(a.dtype)[:] = a.reshape(-1)
    return g


def run_sums(emu, layers, flat, X, prec, min_ws=True, consts=MC.CONSTS, normalize=True, with_fields=False, with_loss=False):
    """(sums [14], fields [4,7,n] or None, loss sums [7] or None) of one call on guarded buffers; the inputs are checked to be unchanged"""
    n = X.shape[0]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    before = [b.raw.copy() for b in [p] + xs]
    wsb = emu.min_workspace_bytes(layers, prec) if min_ws else emu.workspace_bytes(layers, n, prec)
    ws, sws, out = Guarded(wsb), Guarded(emu.material_sums_workspace_bytes()), Guarded(8 * MC.NSUMS, fill=0xFF)
    emu.wave2d_material_sums(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, MC.LB, MC.UB, normalize, *consts, out.ptr, prec, ws.ptr, wsb,
                             sws.ptr, sws.nbytes)
    bufs = [p, ws, sws, out] + xs
    F = L = None
    if with_fields:
        fo = Guarded(4 * 28 * n)
        emu.wave2d_fields(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, MC.LB, MC.UB, normalize, fo.ptr, prec, ws.ptr, wsb)
        F = fo.view(np.float32).reshape(4, 7, n).copy()
        bufs.append(fo)
    if with_loss:
        wl = Guarded(emu.workspace_bytes(layers, n, prec))
        lo, go = Guarded(4 * 8), Guarded(4 * p.nbytes // 4)
        emu.wave2d_loss_grad(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, MC.LB, MC.UB, normalize, *consts, [1.0] * 7, lo.ptr, go.ptr, False,
                             prec, wl.ptr, wl.nbytes)
        L = lo.view(np.float32)[:7].astype(np.float64)
        bufs += [wl, lo, go]
    assert all(b.guards_intact() for b in bufs), "a guard word was overwritten"
    assert all(np.array_equal(b.raw, r) for b, r in zip([p] + xs, before)), "an input was written to"
    return out.view(np.float64).copy(), F, L


@pytest.mark.parametrize("n", MC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", MC.PRIMARY_LINES, ids=[l[0] for l in MC.PRIMARY_LINES])
def test_sums_equal_the_formulas_on_the_fields_call(emu, name, layers, prec, n):
    """PRIMARY check.  Reference: the 14 formulas in float64 on the fp32 output of pinn_wave2d_fields of the same mode; bound: the head's own
    rounding, 8 eps32 S_k (tests/_material_cases.sums_from_fields).  n = 1 and 33 leave one valid point in a tile: a padded lane that added its
    re-read point would show as a multiple of the bound.  n = 2100 runs in the minimum workspace (the fp32 mode then makes several passes)."""
    X = MC.points(n, seed=77)
    s, F, _ = run_sums(emu, layers, MC.fresh_net(tuple(layers)), X, prec, with_fields=True)
    ref, bound, _ = MC.sums_from_fields(F)
    err = np.abs(s - ref)
    print(f"{name} n={n}: max err / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all(), (err / bound)


@pytest.mark.parametrize("name,layers,prec", MC.PRIMARY_LINES, ids=[l[0] for l in MC.PRIMARY_LINES])
def test_sums_of_squares_agree_with_the_loss_call(emu, name, layers, prec):
    """CONSISTENCY: sums[0:7] against loss_terms_out of pinn_wave2d_loss_grad on the same arguments -- two kernels for the same numbers.
    Tolerance: the larger of the primary bound and the fp32 rounding of the loss call's own partial sums, n eps32 sums."""
    n = 2100
    X = MC.points(n, seed=77)
    s, F, L = run_sums(emu, layers, MC.fresh_net(tuple(layers)), X, prec, with_fields=True, with_loss=True)
    _, bound, _ = MC.sums_from_fields(F)
    tol = np.maximum(bound[:7], n * MC.EPS32 * s[:7])
    print(f"{name}: max |sums - loss| / tol = {float((np.abs(s[:7] - L) / tol).max()):.3f}")
    assert (np.abs(s[:7] - L) <= tol).all()


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", MC.SECONDARY_NETS)
def test_sums_against_the_float64_oracle(emu, net, prec):
    """SECONDARY check: max_k |sums_k - oracle_k| / S_k over 1000 collocation points against the float64 oracle's sums, at most 6 x the same metric
    of the oracle run in float32 (the project's convention).  Measured multiples: profiles/material_sums_calls.txt."""
    layers, flat, X, ref, scale, base = MC.secondary_case(net)
    s, _, _ = run_sums(emu, layers, flat, X, prec)
    got = MC.scaled_error(s, ref, scale)
    print(f"{net} {prec}: {got:.3e} = {got / base:.2f} x fp32 oracle {base:.3e}")
    assert got <= 6.0 * base


def test_sums_general_constants_and_raw_inputs(emu):
    """general material constants, plane stress, no input map: against the float64 oracle at fp32-class tolerance of the sums' scale"""
    layers = [3] + 3 * [32] + [7]
    flat = MC.fresh_net(tuple(layers))
    X = MC.points(70, seed=3) / 10.0
    for consts in MC.CONSTS_GENERAL:
        s, _, _ = run_sums(emu, layers, flat, X, "f16x3", consts=consts, normalize=False)
        ref, scale = MC.oracle_sums(flat, layers, X, consts=consts, normalize=False)
        assert MC.scaled_error(s, ref, scale) < 2e-5


def test_sums_packed_flag_empty_set_determinism_and_errors(emu):
    layers = [3] + 4 * [32] + [7]
    flat, X = MC.fresh_net(tuple(layers)), MC.points(33, seed=77)
    n = 33
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb, swb = emu.min_workspace_bytes(layers, "f16x3"), emu.material_sums_workspace_bytes()
    assert swb > 0 and swb % 256 == 0
    ws, sws = Guarded(wsb), Guarded(swb)
    a, b, c = (Guarded(8 * MC.NSUMS, fill=0xFF) for _ in range(3))
    args = lambda out, prec: (p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, MC.LB, MC.UB, True, *MC.CONSTS, out, prec, ws.ptr, wsb, sws.ptr, swb)
    emu.path_counts(reset=True)
    emu.wave2d_material_sums(*args(a.ptr, "f16x3"))
    emu.wave2d_material_sums(*args(b.ptr, "f16x3+packed"))              # the packed weights of the first call are still in the workspace
    ws.view(np.uint8)[:] = 0x5A                                         # a fresh workspace, scratch of other content: the same bits
    sws.view(np.uint8)[:] = 0x5A
    emu.wave2d_material_sums(*args(c.ptr, "f16x3"))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a.view(np.uint64), c.view(np.uint64))
    assert np.isfinite(a.view(np.float64)).all() and (a.view(np.float64)[:7] > 0).all()
    wsf = Guarded(emu.min_workspace_bytes(layers, "fp32"))
    emu.wave2d_material_sums(*(args(b.ptr, "fp32")[:-4] + (wsf.ptr, wsf.nbytes, sws.ptr, swb)))
    assert not any(emu.path_counts().values()) and wsf.guards_intact()   # not a loss + gradient call: no path counter moves, in any mode
    L, C = emu.lib, ctypes
    li, d3 = (C.c_int * len(layers))(*layers), (C.c_double * 3)
    raw = lambda n_, out=a.ptr, w_=ws.ptr, wb=wsb, sw=sws.ptr, sb=swb, lay=li, nl=len(layers), prec=1, x_=xs[0].ptr: L.pinn_wave2d_material_sums(
        p.ptr, lay, nl, x_, xs[1].ptr, xs[2].ptr, n_, d3(*MC.LB), d3(*MC.UB), 1, 2.5, 0.25, 1.0, 1, out, prec, w_, wb, sw, sb, None)
    for prec in (1, 4):                                                 # n == 0 writes 14 zeros
        a.view(np.uint8)[:] = 0xFF
        assert raw(0, prec=prec) == 0 and raw(0, prec=prec, x_=None) == 0 and not a.view(np.uint64).any()
    assert raw(-1) == -5
    assert raw(n, out=None) == -1 and raw(n, w_=None) == -1 and raw(n, sw=None) == -1 and raw(n, x_=None) == -1 and raw(0, out=None) == -1
    assert raw(n, wb=256) == -4 and raw(n, w_=ws.ptr + 16) == -4 and raw(n, sb=swb - 1) == -4 and raw(n, sw=sws.ptr + 16) == -4
    assert raw(n, prec=77) == -3
    five = [3, 32, 32, 5]
    assert raw(n, lay=(C.c_int * 4)(*five), nl=4) == -2                 # not the seven outputs of the wave net
    assert all(g.guards_intact() for g in [p, ws, sws, a, b, c] + xs)
