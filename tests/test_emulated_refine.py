"""CPU tests of the refinement calls (pinn_wave2d_residual_score, pinn_select_k): the kernel sources compiled for x86 against the SIMT emulator, on host
arrays framed by guard words that are checked after every call (as in test_emulated_lbfgs.py).  Selection is compared for exact equality with a numpy
reference; the score against the library's own fields call (head rounding only) and against the float64 oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _refine_cases as RC

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


# ---- selection ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.SELECT_DATA)
@pytest.mark.parametrize("n", RC.SELECT_N)
def test_select_k_equals_the_numpy_reference(emu, n, kind):
    """every k of {0, 1, n // 10, n - 1, n}, both directions: the indices equal the reference's exactly; no byte outside the buffers changes"""
    score = RC.select_data(kind, n)
    sc, ws = put(score), Guarded(emu.select_workspace_bytes(n))
    for k in RC.select_ks(n):
        for largest in (True, False):
            out = Guarded(4 * k, fill=0xFF)
            emu.select_k(sc.ptr, n, k, largest, out.ptr, ws.ptr, ws.nbytes)
            assert sc.guards_intact() and ws.guards_intact() and out.guards_intact(), "a guard word was overwritten"
            assert np.array_equal(sc.view(np.uint32), score.view(np.uint32)), "the scores were written to"
            assert np.array_equal(out.view(np.int32), RC.select_reference(score, k, largest)), (n, k, largest, kind)


def test_select_k_argument_errors(emu):
    L = emu.lib
    nb = emu.select_workspace_bytes(100)
    assert nb > 0 and emu.select_workspace_bytes(-1) == 0 and emu.select_workspace_bytes(1 << 31) == 0 and emu.select_workspace_bytes((1 << 31) - 1) == nb
    sc, ws, out = put(np.arange(100, dtype=np.float32)), Guarded(nb), Guarded(400)
    call = lambda n, k, w=ws.ptr, wb=nb, s=sc.ptr, o=out.ptr: L.pinn_select_k(s, n, k, 1, o, w, wb, None)
    assert call(1 << 31, 1) == -5 and call(-1, 0) == -5 and call(100, 101) == -5 and call(100, -1) == -5
    assert call(100, 10, wb=nb - 1) == -4 and call(100, 10, w=ws.ptr + 16) == -4
    assert call(100, 10, w=None) == -1 and call(100, 10, s=None) == -1 and call(100, 10, o=None) == -1
    before = out.raw.copy()
    assert call(100, 0) == 0 and call(0, 0, s=None, o=None) == 0               # valid no-ops
    assert np.array_equal(before, out.raw) and ws.guards_intact() and sc.guards_intact()
    assert call(100, 10) == 0 and np.array_equal(out.view(np.int32)[:10], np.arange(90, 100))


# ---- score -------------------------------------------------------------------------------------------------------------------------------------
def run_score(emu, layers, flat, X, prec, w=RC.WEIGHTS, min_ws=True, consts=(2.5, 0.25, 1.0, True), normalize=True, with_fields=False):
    n = X.shape[0]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, prec) if min_ws else emu.workspace_bytes(layers, n, prec)
    ws, out = Guarded(wsb), Guarded(4 * n, fill=0xFF)
    emu.wave2d_residual_score(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, RC.LB, RC.UB, normalize, *consts, w, out.ptr, prec, ws.ptr, wsb)
    bufs = [p, ws, out] + xs
    F = None
    if with_fields:
        fo = Guarded(4 * 28 * n)
        emu.wave2d_fields(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, RC.LB, RC.UB, normalize, fo.ptr, prec, ws.ptr, wsb)
        F = fo.view(np.float32).reshape(4, 7, n).copy()
        bufs.append(fo)
    assert all(b.guards_intact() for b in bufs), "a guard word was overwritten"
    return out.view(np.float32).copy(), F


@pytest.mark.parametrize("n", RC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", RC.PRIMARY_LINES, ids=[l[0] for l in RC.PRIMARY_LINES])
def test_score_equals_the_residuals_of_the_fields_call(emu, name, layers, prec, n):
    """PRIMARY check.  Reference: the residual formulas in float64 on the fp32 output of pinn_wave2d_fields of the same mode; bound: the head's own
    rounding, 16 eps32 sum_i w_i a_i^2 per point (tests/_refine_cases.score_from_fields).  That presumes the forward of the two heads is the same
    bit for bit -- it is the same template code; the bound holding at every line and size is the evidence.  n = 2100 runs in the minimum workspace
    (the fp32 mode then walks the points in nine passes; the 16-bit families need no panels for a forward-only head and make one launch)."""
    X = RC.points(n, seed=77)
    s, F = run_score(emu, layers, RC.fresh_net(tuple(layers)), X, prec, with_fields=True)
    ref, bound = RC.score_from_fields(F)
    err = np.abs(s.astype(np.float64) - ref)
    print(f"{name} n={n}: max |delta| / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all()


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", RC.SECONDARY_NETS)
def test_score_against_the_float64_oracle(emu, net, prec):
    """SECONDARY check: relative L2 error of s and of sqrt(s) over 1000 collocation points (box minus source disc, see _refine_cases.collocation_set
    for why not uniform points) against the float64 residuals of the oracle, at most 6 x the same metric of the oracle evaluated in float32 (the
    project's per-layer convention).  Measured multiples, emulator build: fresh 4x32 1.5 / 1.2 (f16x3 / fp32), fresh 8x64 1.6 / 1.8, trained
    inf20s 1.25 / 1.3; on the GPU: profiles/residual_score_accuracy.txt."""
    layers, flat, X, ref, base = RC.secondary_case(net)
    s, _ = run_score(emu, layers, flat, X, prec)
    got = (RC.rel_l2(s, ref), RC.rel_l2(np.sqrt(s.astype(np.float64)), np.sqrt(ref)))
    print(f"{net} {prec}: s {got[0]:.3e} ({got[0] / base[0]:.2f} x fp32 oracle {base[0]:.3e}), sqrt(s) {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


def test_score_constants_weights_and_raw_inputs(emu):
    """general material constants, plane stress, no input map, weights with zeros: against the float64 oracle at fp32-class tolerance"""
    layers = [3] + 3 * [32] + [7]
    flat = RC.fresh_net(tuple(layers))
    X = RC.points(70, seed=3) / 10.0
    w = (0.0, 1.5, 0.0, 2.0, 1.0, 0.0, 0.25)
    for consts in ((7.3, 0.31, 1.9, True), (7.3, 0.31, 1.9, False)):
        s, _ = run_score(emu, layers, flat, X, "f16x3", w=w, consts=consts, normalize=False)
        ref = RC.oracle_score(flat, layers, X, w=w, normalize=False, E=consts[0], mu=consts[1], rho=consts[2], plane_strain=consts[3])
        assert RC.rel_l2(s, ref) < 2e-5


def test_score_packed_flag_empty_set_and_errors(emu):
    layers = [3] + 4 * [32] + [7]
    flat, X = RC.fresh_net(tuple(layers)), RC.points(33, seed=77)
    n = 33
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, "f16x3")
    ws, a, b = Guarded(wsb), Guarded(4 * n, fill=0xFF), Guarded(4 * n, fill=0xFF)
    args = lambda out, prec: (p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, RC.LB, RC.UB, True, 2.5, 0.25, 1.0, True, RC.WEIGHTS, out, prec, ws.ptr, wsb)
    emu.path_counts(reset=True)
    emu.wave2d_residual_score(*args(a.ptr, "f16x3"))
    emu.wave2d_residual_score(*args(b.ptr, "f16x3+packed"))             # the packed weights of the first call are still in the workspace
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a.view(np.float32)).all()
    wsf = Guarded(emu.min_workspace_bytes(layers, "fp32"))
    emu.wave2d_residual_score(*(args(b.ptr, "fp32")[:-2] + (wsf.ptr, wsf.nbytes)))
    assert not any(emu.path_counts().values()) and wsf.guards_intact()   # not a loss + gradient call: no path counter moves, in any mode
    L, C = emu.lib, ctypes
    li, d3 = (C.c_int * len(layers))(*layers), (C.c_double * 3)
    tw = (C.c_float * 7)(*RC.WEIGHTS)
    raw = lambda n_, out=a.ptr, w_=ws.ptr, wb=wsb, tw_=tw, lay=li, nl=len(layers), prec=1: L.pinn_wave2d_residual_score(
        p.ptr, lay, nl, xs[0].ptr, xs[1].ptr, xs[2].ptr, n_, d3(*RC.LB), d3(*RC.UB), 1, 2.5, 0.25, 1.0, 1, tw_, out, prec, w_, wb, None)
    before = a.raw.copy()
    assert raw(0) == 0 and raw(0, out=None) == 0 and np.array_equal(before, a.raw)                    # n == 0: a valid no-op
    assert raw(-1) == -5 and raw(n, out=None) == -1 and raw(n, tw_=None) == -1 and raw(n, w_=None) == -1
    assert raw(n, wb=256) == -4 and raw(n, w_=ws.ptr + 16) == -4 and raw(n, prec=77) == -3
    five = [3, 32, 32, 5]
    assert raw(n, lay=(C.c_int * 4)(*five), nl=4) == -2                  # not the seven outputs of the wave net
    assert all(g.guards_intact() for g in [p, ws, a, b] + xs)
