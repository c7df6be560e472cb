"""CPU tests of the predict heads (pinn_wave2d_predict, pinn_plate2d_predict) and of pinn_field_error_sums: the kernel
sources compiled for x86 against the SIMT emulator, on host arrays framed by guard words that are checked after every call.  The predict
output against the library's own fields / streams call (head rounding only), against the float64 reference, the error sums against numpy,
and the conventions of the C-ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _predict_cases as PC
from tests._predict_cases import Guarded, put

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, stdout=subprocess.DEVNULL)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


def run(emu, family, layers, flat, X, prec, frozen=None, with_fields=False):
    """predict in the MINIMUM workspace (and the fields / streams call of the same net and mode).  Returns (out [rows, n], fields or None)."""
    n, din = X.shape[0], X.shape[1]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(din)]
    cols = [c.ptr for c in xs]
    wsb = emu.min_workspace_bytes(layers, prec)
    rows = 8
    ws, out = Guarded(wsb), Guarded(4 * rows * n, fill=0xFF)
    bufs = [p, ws, out] + xs
    fr = None
    if family == "wave":
        emu.wave2d_predict(p.ptr, layers, *cols, n, PC.LB, PC.UB, True, out.ptr, prec, ws.ptr, wsb)
    else:
        fr = put(np.ascontiguousarray(frozen, dtype=np.float32))
        bufs.append(fr)
        emu.plate2d_predict(p.ptr, layers, *cols, n, PC.PLATE_LB, PC.PLATE_UB, False, fr.ptr, out.ptr, prec, ws.ptr, wsb)
    F = None
    if with_fields:
        ns = 4 if family == "wave" else 5
        fo = Guarded(4 * ns * layers[-1] * n)
        bufs.append(fo)
        if family == "wave":
            emu.wave2d_fields(p.ptr, layers, *cols, n, PC.LB, PC.UB, True, fo.ptr, prec, ws.ptr, wsb)
        else:
            emu.net_streams(p.ptr, layers, *cols, n, PC.PLATE_LB, PC.PLATE_UB, False, fo.ptr, prec, ws.ptr, wsb)
        F = fo.view(np.float32).reshape(ns, layers[-1], n).copy()
    assert all(b.guards_intact() for b in bufs), "a guard word was overwritten"
    if fr is not None:
        assert np.array_equal(fr.view(np.uint32), np.ascontiguousarray(frozen, dtype=np.float32).reshape(-1).view(np.uint32)), "the frozen streams were written to"
    return out.view(np.float32).reshape(rows, n).copy(), F


def streams_of(emu, layers, flat, X, prec):
    n = X.shape[0]
    p = put(np.asarray(flat, dtype=np.float32))
    xs = [put(X[:, k].astype(np.float32)) for k in range(3)]
    wsb = emu.min_workspace_bytes(layers, prec)
    ws, so = Guarded(wsb), Guarded(4 * 5 * layers[-1] * n)
    emu.net_streams(p.ptr, layers, xs[0].ptr, xs[1].ptr, xs[2].ptr, n, PC.PLATE_LB, PC.PLATE_UB, False, so.ptr, prec, ws.ptr, wsb)
    assert so.guards_intact() and ws.guards_intact()
    return so.view(np.float32).reshape(5, layers[-1], n).copy()


def check_primary(tag, out, ref, bound):
    err = np.abs(out.astype(np.float64) - ref)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{tag}: max |delta| / bound = {worst:.3f}")
    assert np.isfinite(out).all() and (err <= bound).all()


# ---- primary: head and stream subset against the library's own fields call --------------------------------------------------------------------------
@pytest.mark.parametrize("n", PC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", PC.WAVE_LINES, ids=[l[0] for l in PC.WAVE_LINES])
def test_wave_predict_equals_the_rows_of_the_fields_call(emu, name, layers, prec, n):
    """PRIMARY check.  Reference: the predict formulas in float64 on the fp32 output of pinn_wave2d_fields of the same net and mode; bound
    4 eps32 x (sum of the absolute values of the row's leaf terms) per point (_predict_cases states the count); no slack for the forward: the
    three carried streams run the per-stream instructions of the four-stream call."""
    X = PC.wave_points(n)
    out, F = run(emu, "wave", layers, PC.fresh_net(tuple(layers)), X, prec, with_fields=True)
    check_primary(f"wave {name} n={n}", out, *PC.wave_predict_from_fields(F))


@pytest.mark.parametrize("n", PC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", PC.PLATE_LINES, ids=[l[0] for l in PC.PLATE_LINES])
def test_plate_predict_equals_the_composite_of_the_streams_call(emu, name, layers, prec, n):
    """PRIMARY check of the plate head: composite formulas in float64 on the fp32 output of pinn_net_streams and the fp32 frozen streams passed
    in.  Stream rows 3 and 4 of both frozen blocks are NaN: the output must be finite and within the bound, the frozen array unchanged."""
    X, fr = PC.plate_uniform(n), PC.poisoned(PC.plate_frozen(n))
    out, N = run(emu, "plate", layers, PC.fresh_net(tuple(layers)), X, prec, frozen=fr, with_fields=True)
    check_primary(f"plate {name} n={n}", out, *PC.plate_predict_from_streams(N, fr))


# ---- secondary: the float64 reference -------------------------------------------------------------------------------------------------------------------
def test_float32_reference_errors_are_usable():
    """the bar of the secondary check divides by the float32 reference's own block errors: nonzero and finite for every case"""
    for fam, net in PC.SECONDARY_CASES:
        base = PC.secondary_case(fam, net)[4]
        print(f"{fam} {net}: float32 reference value block {base[0]:.3e}, strain block {base[1]:.3e}")
        assert all(np.isfinite(b) and b > 0.0 for b in base), (fam, net, base)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("family,net", PC.SECONDARY_CASES, ids=[f"{f}-{n}" for f, n in PC.SECONDARY_CASES])
def test_predict_against_the_float64_reference(emu, family, net, prec):
    """SECONDARY check: relative L2 over 1000 points of the value rows as one block and of the strain rows as one block against the float64
    reference formulas, at most 6 x the same error of the reference run in float32.  Plate: D / P are the library's own pinn_net_streams of the
    trained distance / particular nets in the same mode.  On the GPU: profiles/predict_head_accuracy.txt."""
    layers, flat, X, ref, base = PC.secondary_case(family, net)
    frozen = None
    if family == "plate":
        ld, fd = PC.golden_net("plate_dist")
        lp, fp = PC.golden_net("plate_part")
        frozen = np.stack([streams_of(emu, ld, fd, X, prec), streams_of(emu, lp, fp, X, prec)])
    out, _ = run(emu, family, layers, flat, X, prec, frozen=frozen)
    got = PC.block_errors(family, out, ref)
    print(f"{family} {net} {prec}: values {got[0]:.3e} ({got[0] / base[0]:.2f} x float32 reference {base[0]:.3e}), "
          f"strains {got[1]:.3e} ({got[1] / base[1]:.2f} x {base[1]:.3e})")
    assert got[0] <= 6.0 * base[0] and got[1] <= 6.0 * base[1]


# ---- pinn_field_error_sums ----------------------------------------------------------------------------------------------------------------------------------
def error_sums(emu, pred, ref, rows=PC.ERR_ROWS):
    n = ref.shape[1]
    wsb = emu.field_error_workspace_bytes(n, len(rows))
    assert wsb > 0
    gp, gr, ws, out = put(pred), put(ref), Guarded(wsb), Guarded(8 * 2 * len(rows), fill=0xFF)
    emu.field_error_sums(gp.ptr, pred.shape[0], rows, gr.ptr, n, out.ptr, ws.ptr, wsb)
    assert all(g.guards_intact() for g in (gp, gr, ws, out))
    return out.view(np.float64).reshape(2, len(rows)).copy()


@pytest.mark.parametrize("n", PC.ERR_N)
def test_field_error_sums_against_numpy(emu, n):
    """sum (pred[rows[j]] - ref[j])^2 and sum ref[j]^2 against numpy float64 on the same fp32 arrays: relative difference <= (n + 2) 2^-52 per sum
    (fp64 differences and squares, n additions in any order); two calls give identical bits; the rows that are not selected are NaN"""
    pred, ref, want = PC.error_data(n)
    a, b = error_sums(emu, pred, ref), error_sums(emu, pred, ref)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if n == 0:
        assert (a == 0.0).all()
        return
    rel = np.abs(a - want) / want
    print(f"error sums n={n}: largest relative difference {rel.max():.2e} (bound {(n + 2) * 2.0 ** -52:.2e})")
    assert (rel <= (n + 2) * 2.0 ** -52).all()


def test_field_error_sums_error_codes(emu):
    """every error code without device work; the workspace size of a rejected n is 0"""
    L, C = emu.lib, ctypes
    n = 33
    pred, ref, _ = PC.error_data(n)
    gp, gr, ws, out = put(pred), put(ref), Guarded(emu.field_error_workspace_bytes(n, 3)), Guarded(8 * 6, fill=0xFF)
    rows = (C.c_int * 3)(*PC.ERR_ROWS)
    raw = lambda n_=n, pr=gp.ptr, prows=8, rw=rows, nr=3, rf=gr.ptr, so=out.ptr, w_=ws.ptr, wb=ws.nbytes: L.pinn_field_error_sums(
        pr, prows, rw, nr, rf, n_, so, w_, wb, None)
    before = out.raw.copy()
    assert raw(n_=-1) == -5 and raw(n_=1 << 31) == -5 and raw(nr=0) == -5 and raw(nr=17) == -5 and raw(prows=0) == -5
    assert raw(rw=(C.c_int * 3)(0, 8, 4)) == -5 and raw(rw=(C.c_int * 3)(0, -1, 4)) == -5 and raw(prows=4) == -5
    assert raw(pr=None) == -1 and raw(rf=None) == -1 and raw(so=None) == -1 and raw(w_=None) == -1 and raw(rw=None) == -1
    assert raw(wb=ws.nbytes - 1) == -4 and raw(w_=ws.ptr + 16) == -4
    assert np.array_equal(before, out.raw) and all(g.guards_intact() for g in (gp, gr, ws, out))
    assert emu.field_error_workspace_bytes(-1, 3) == 0 and emu.field_error_workspace_bytes(1 << 31, 3) == 0
    assert emu.field_error_workspace_bytes(n, 0) == 0 and emu.field_error_workspace_bytes(n, 17) == 0
    assert emu.field_error_workspace_bytes(0, 16) >= emu.field_error_workspace_bytes(0, 1) > 0


# ---- the C-ABI's conventions, per predict call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["wave", "plate"])
def test_predict_packed_flag_empty_set_and_errors(emu, family):
    from pinn_elastodynamics_amd.capi import PREC
    din, nout, rows = {"wave": (3, 7, 8), "plate": (3, 5, 8)}[family]
    layers = [din] + 3 * [32] + [nout]
    n = 33
    flat = PC.fresh_net(tuple(layers))
    X = {"wave": PC.wave_points, "plate": PC.plate_uniform}[family](n)
    lb, ub, norm = {"wave": (PC.LB, PC.UB, 1), "plate": (PC.PLATE_LB, PC.PLATE_UB, 0)}[family]
    p = put(np.asarray(flat, dtype=np.float32))
    fr = put(PC.plate_frozen(n))
    xs = [put(X[:, k].astype(np.float32)) for k in range(din)]
    wsb = emu.min_workspace_bytes(layers, "f16x3")
    ws, a, b = Guarded(wsb), Guarded(4 * rows * n, fill=0xFF), Guarded(4 * rows * n, fill=0xFF)
    L, C = emu.lib, ctypes
    dd = (C.c_double * din)
    fn = getattr(L, {"wave": "pinn_wave2d_predict", "plate": "pinn_plate2d_predict"}[family])

    def raw(n_, out=a.ptr, w_=ws.ptr, wb=wsb, lay=layers, prec=PREC["f16x3"], fz=fr.ptr):
        li = (C.c_int * len(lay))(*lay)
        mid = (fz,) if family == "plate" else ()
        return fn(p.ptr, li, len(lay), *[c.ptr for c in xs], n_, dd(*lb), dd(*ub), norm, *mid, out, prec, w_, wb, None)

    emu.path_counts(reset=True)
    assert raw(n) == 0 and raw(n, out=b.ptr, prec=PREC["f16x3+packed"]) == 0      # the packed weights of the first call are still in the workspace
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a.view(np.float32)).all()
    wsf = Guarded(emu.min_workspace_bytes(layers, "fp32"))
    assert raw(n, out=b.ptr, prec=PREC["fp32"], w_=wsf.ptr, wb=wsf.nbytes) == 0
    assert not any(emu.path_counts().values()) and wsf.guards_intact()            # no path counter moves, in any mode
    before = a.raw.copy()
    assert raw(0) == 0 and raw(0, out=None, fz=None) == 0 and np.array_equal(before, a.raw)            # n == 0 touches nothing
    assert raw(-1) == -5 and raw(n, out=None) == -1 and raw(n, w_=None) == -1
    if family == "plate":
        assert raw(n, fz=None) == -1
    assert raw(n, wb=256) == -4 and raw(n, w_=ws.ptr + 16) == -4 and raw(n, prec=77) == -3
    l64 = [din, 64, 64, nout]                                                      # (a width every mode is compiled for)
    one_mfma = 0 if family == "wave" else -3                                       # the plate head: split modes only
    w64 = Guarded(emu.min_workspace_bytes(l64, "f16"))
    assert raw(n, out=b.ptr, prec=PREC["f16"], lay=l64, w_=w64.ptr, wb=w64.nbytes) == one_mfma
    assert raw(n, out=b.ptr, prec=PREC["bf16"], lay=l64, w_=w64.ptr, wb=w64.nbytes) == one_mfma
    assert raw(n, lay=[din, 32, 32, nout + 1]) == -2 and raw(n, lay=[7 - din, 32, 32, nout]) == -2
    assert np.array_equal(before, a.raw) and all(g.guards_intact() for g in [p, fr, ws, a, b, w64] + xs)
