"""CPU tests of pinn_plate2d_residual_score and pinn_nc3d_residual_score: the kernel sources compiled for x86 against the SIMT emulator, on host
arrays framed by guard words that are checked after every call (as in test_emulated_refine.py).  The score against the library's own streams /
fields call (head rounding only), against the float64 oracle, and the conventions of the C-ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _refine_family_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, stdout=subprocess.DEVNULL)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


class Guarded:
    """nbytes of payload at a 256-byte aligned address, guard words in front and behind"""

    def __init__(self, nbytes, fill=0xA5):
        self.raw = np.full(nbytes + 2 * GUARD + 512, 0xA5, dtype=np.uint8)
        base = self.raw.ctypes.data
        self.off = (-(base + GUARD) % 256) + GUARD
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


def run_plate(emu, layers, flat, X, frozen, prec, w=FC.PLATE_WEIGHTS, with_streams=False):
    """score in the MINIMUM workspace (and the streams of the same net and mode); frozen: fp32 [2,5,5,n]"""
    n = X.shape[0]
    p, fr = put(np.asarray(flat, dtype=np.float32)), put(np.ascontiguousarray(frozen, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, prec)
    ws, out = Guarded(wsb), Guarded(4 * n, fill=0xFF)
    emu.plate2d_residual_score(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, FC.PLATE_LB, FC.PLATE_UB, False, fr.ptr, 20.0, 0.25, 1.0, w,
                               out.ptr, prec, ws.ptr, wsb)
    bufs = [p, fr, ws, out] + xs
    N = None
    if with_streams:
        so = Guarded(4 * 25 * n)
        emu.net_streams(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, FC.PLATE_LB, FC.PLATE_UB, False, so.ptr, prec, ws.ptr, wsb)
        N = so.view(np.float32).reshape(5, 5, n).copy()
        bufs.append(so)
    assert all(b.guards_intact() for b in bufs), "a guard word was overwritten"
    assert np.array_equal(fr.view(np.float32), np.asarray(frozen, dtype=np.float32).reshape(-1)), "the frozen streams were written to"
    return out.view(np.float32).copy(), N


def streams_of(emu, layers, flat, X, prec):
    n = X.shape[0]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, prec)
    ws, so = Guarded(wsb), Guarded(4 * 5 * layers[-1] * n)
    emu.net_streams(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, FC.PLATE_LB, FC.PLATE_UB, False, so.ptr, prec, ws.ptr, wsb)
    assert so.guards_intact() and ws.guards_intact()
    return so.view(np.float32).reshape(5, layers[-1], n).copy()


def run_nc3d(emu, layers, flat, X, prec, w=FC.NC3D_WEIGHTS, with_fields=False):
    n = X.shape[0]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(4)]
    wsb = emu.min_workspace_bytes(layers, prec)
    ws, out = Guarded(wsb), Guarded(4 * n, fill=0xFF)
    emu.nc3d_residual_score(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, xs[3].ptr, n, FC.NC3D_LB, FC.NC3D_UB, True, 2.5, 0.25, 1.0, w, out.ptr,
                            prec, ws.ptr, wsb)
    bufs = [p, ws, out] + xs
    F = None
    if with_fields:
        fo = Guarded(4 * 60 * n)
        emu.nc3d_fields(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, xs[3].ptr, n, FC.NC3D_LB, FC.NC3D_UB, True, fo.ptr, prec, ws.ptr, wsb)
        F = fo.view(np.float32).reshape(5, 12, n).copy()
        bufs.append(fo)
    assert all(b.guards_intact() for b in bufs), "a guard word was overwritten"
    return out.view(np.float32).copy(), F


# ---- primary: head rounding only ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", FC.PLATE_LINES, ids=[l[0] for l in FC.PLATE_LINES])
def test_plate_score_equals_the_residuals_of_the_streams_call(emu, name, layers, prec, n):
    """PRIMARY check.  Reference: composite and residual formulas in float64 on the fp32 output of pinn_net_streams of the same mode and the
    exact fp32 frozen streams passed in; bound 24 eps32 sum_i |w_i| a_i^2 per point over the leaf terms
    (_refine_family_cases.plate_score_from_streams states the count).  n = 2100 in the minimum workspace: the fp32 mode walks several passes."""
    X, fr = FC.plate_uniform(n), FC.plate_frozen(n)
    s, N = run_plate(emu, layers, FC.fresh_net(tuple(layers)), X, fr, prec, with_streams=True)
    ref, bound = FC.plate_score_from_streams(N, fr)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"plate {name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()


@pytest.mark.parametrize("n", FC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", FC.NC3D_LINES, ids=[l[0] for l in FC.NC3D_LINES])
def test_nc3d_score_equals_the_residuals_of_the_fields_call(emu, name, layers, prec, n):
    """PRIMARY check of the 3-D head: float64 residual formulas on the fp32 output of pinn_nc3d_fields of the same mode, bound
    24 eps32 sum_i |w_i| a_i^2 (_refine_family_cases.nc3d_score_from_fields).  All seven lines are accepted for four inputs."""
    assert emu.workspace_bytes(layers, n, prec) > 0
    X = FC.nc3d_points(n)
    s, F = run_nc3d(emu, layers, FC.fresh_net(tuple(layers)), X, prec, with_fields=True)
    ref, bound = FC.nc3d_score_from_fields(F)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"nc3d {name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()


# ---- secondary: the float64 oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", FC.PLATE_SECONDARY)
def test_plate_score_against_the_float64_oracle(emu, net, prec):
    """SECONDARY check: relative L2 of s and of sqrt(s) over 1000 plate collocation points (seed 1111) against the float64 oracle (net_streams ->
    composite -> plate_residuals, D and P from the trained nets), at most 6 x the same metric of the oracle run in float32.  The frozen streams
    the call gets are the library's own pinn_net_streams of the trained D / P nets in the same mode, as the class computes them.
    Measured multiples, emulator build (s / sqrt(s)): f16x3 fresh 4x32 0.85 / 1.11, trained 8x70 1.59 / 2.10, trained 8x64 2.29 / 3.17;
    fp32 0.87 / 1.01, 0.86 / 0.87, 1.03 / 1.18; on the GPU: profiles/residual_score_accuracy.txt."""
    layers, flat, X, ref, base = FC.plate_secondary_case(net)
    ld, fd = FC.golden_net("plate_dist")
    lp, fp = FC.golden_net("plate_part")
    frozen = np.stack([streams_of(emu, ld, fd, X, prec), streams_of(emu, lp, fp, X, prec)])
    s, _ = run_plate(emu, layers, flat, X, frozen, prec, w=FC.PLATE_DEFAULT_W)
    got = (FC.rel_l2(s, ref), FC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"plate {net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", FC.NC3D_SECONDARY)
def test_nc3d_score_against_the_float64_oracle(emu, net, prec):
    """SECONDARY check of the 3-D head: nc3d_fields -> nc3d_residuals in float64 over 1000 half-space points, bar 6 x the float32 oracle's own error.
    Measured multiples, emulator build (s / sqrt(s)): f16x3 fresh 3x32 1.27 / 1.30, fresh 10x128 1.07 / 1.07; fp32 1.56 / 1.57, 1.74 / 1.74;
    on the GPU: profiles/residual_score_accuracy.txt."""
    layers, flat, X, ref, base = FC.nc3d_secondary_case(net)
    s, _ = run_nc3d(emu, layers, flat, X, prec, w=FC.NC3D_DEFAULT_W)
    got = (FC.rel_l2(s, ref), FC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"nc3d {net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


# ---- the C-ABI's conventions ------------------------------------------------------------------------------------------------------------------------
def test_plate_score_packed_flag_empty_set_and_errors(emu):
    layers = [3] + 4 * [32] + [5]
    n = 33
    flat, X, frz = FC.fresh_net(tuple(layers)), FC.plate_uniform(n), FC.plate_frozen(n)
    p, fr = put(np.asarray(flat, dtype=np.float32)), put(np.ascontiguousarray(frz))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, "f16x3")
    ws, a, b = Guarded(wsb), Guarded(4 * n, fill=0xFF), Guarded(4 * n, fill=0xFF)
    args = lambda out, prec: (p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, FC.PLATE_LB, FC.PLATE_UB, False, fr.ptr, 20.0, 0.25, 1.0,
                              FC.PLATE_WEIGHTS, out, prec, ws.ptr, wsb)
    emu.path_counts(reset=True)
    emu.plate2d_residual_score(*args(a.ptr, "f16x3"))
    emu.plate2d_residual_score(*args(b.ptr, "f16x3+packed"))            # the packed weights of the first call are still in the workspace
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a.view(np.float32)).all()
    wsf = Guarded(emu.min_workspace_bytes(layers, "fp32"))
    emu.plate2d_residual_score(*(args(b.ptr, "fp32")[:-2] + (wsf.ptr, wsf.nbytes)))
    assert not any(emu.path_counts().values()) and wsf.guards_intact()  # not a loss + gradient call: no path counter moves, in any mode
    L, C = emu.lib, ctypes
    li, d3 = (C.c_int * len(layers))(*layers), (C.c_double * 3)
    tw = (C.c_float * 5)(*FC.PLATE_WEIGHTS)
    raw = lambda n_, out=a.ptr, w_=ws.ptr, wb=wsb, tw_=tw, lay=li, nl=len(layers), prec=1, fz=fr.ptr: L.pinn_plate2d_residual_score(
        p.ptr, lay, nl, xs[0].ptr, xs[1].ptr, xs[2].ptr, n_, d3(*FC.PLATE_LB), d3(*FC.PLATE_UB), 0, fz, 20.0, 0.25, 1.0, tw_, out, prec, w_, wb, None)
    from pinn_elastodynamics_amd.capi import PREC
    before = a.raw.copy()
    assert raw(0) == 0 and raw(0, out=None, fz=None) == 0 and np.array_equal(before, a.raw)            # n == 0: a valid no-op
    assert raw(-1) == -5 and raw(n, out=None) == -1 and raw(n, tw_=None) == -1 and raw(n, fz=None) == -1 and raw(n, w_=None) == -1
    assert raw(n, wb=256) == -4 and raw(n, w_=ws.ptr + 16) == -4 and raw(n, prec=77) == -3
    l64 = dict(lay=(C.c_int * 4)(3, 64, 64, 5), nl=4)                                                  # (a width every mode is compiled for)
    assert raw(n, prec=PREC["f16"], **l64) == -3 and raw(n, prec=PREC["bf16"], **l64) == -3           # the non-split modes, as the loss call
    assert raw(n, lay=(C.c_int * 4)(3, 32, 32, 7), nl=4) == -2                                        # not the five outputs of the plate net
    assert raw(n, lay=(C.c_int * 4)(4, 32, 32, 5), nl=4) == -2                                        # not three inputs
    assert np.array_equal(before, a.raw) and all(g.guards_intact() for g in [p, fr, ws, a, b] + xs)


def test_nc3d_score_packed_flag_empty_set_and_errors(emu):
    layers = [4] + 3 * [32] + [12]
    n = 33
    flat, X = FC.fresh_net(tuple(layers)), FC.nc3d_points(n)
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(4)]
    wsb = emu.min_workspace_bytes(layers, "f16x3")
    ws, a, b = Guarded(wsb), Guarded(4 * n, fill=0xFF), Guarded(4 * n, fill=0xFF)
    args = lambda out, prec: (p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, xs[3].ptr, n, FC.NC3D_LB, FC.NC3D_UB, True, 2.5, 0.25, 1.0,
                              FC.NC3D_WEIGHTS, out, prec, ws.ptr, wsb)
    emu.path_counts(reset=True)
    emu.nc3d_residual_score(*args(a.ptr, "f16x3"))
    emu.nc3d_residual_score(*args(b.ptr, "f16x3+packed"))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a.view(np.float32)).all()
    wsf = Guarded(emu.min_workspace_bytes(layers, "fp32"))
    emu.nc3d_residual_score(*(args(b.ptr, "fp32")[:-2] + (wsf.ptr, wsf.nbytes)))
    assert not any(emu.path_counts().values()) and wsf.guards_intact()
    L, C = emu.lib, ctypes
    li, d4 = (C.c_int * len(layers))(*layers), (C.c_double * 4)
    tw = (C.c_float * 12)(*FC.NC3D_WEIGHTS)
    raw = lambda n_, out=a.ptr, w_=ws.ptr, wb=wsb, tw_=tw, lay=li, nl=len(layers), prec=1: L.pinn_nc3d_residual_score(
        p.ptr, lay, nl, xs[0].ptr, xs[1].ptr, xs[2].ptr, xs[3].ptr, n_, d4(*FC.NC3D_LB), d4(*FC.NC3D_UB), 1, 2.5, 0.25, 1.0, tw_, out, prec, w_, wb,
        None)
    from pinn_elastodynamics_amd.capi import PREC
    before = a.raw.copy()
    assert raw(0) == 0 and raw(0, out=None) == 0 and np.array_equal(before, a.raw)
    assert raw(-1) == -5 and raw(n, out=None) == -1 and raw(n, tw_=None) == -1 and raw(n, w_=None) == -1
    assert raw(n, wb=256) == -4 and raw(n, w_=ws.ptr + 16) == -4 and raw(n, prec=77) == -3
    l64 = dict(lay=(C.c_int * 4)(4, 64, 64, 12), nl=4)
    assert raw(n, prec=PREC["f16"], **l64) == -3 and raw(n, prec=PREC["bf16"], **l64) == -3           # the non-split modes, as the loss call
    assert raw(n, lay=(C.c_int * 4)(4, 32, 32, 7), nl=4) == -2                                        # not twelve outputs
    assert raw(n, lay=(C.c_int * 4)(3, 32, 32, 12), nl=4) == -2                                       # not four inputs
    assert np.array_equal(before, a.raw) and all(g.guards_intact() for g in [p, ws, a, b] + xs)
