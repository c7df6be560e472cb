"""CPU tests of pinn_stream_loss_grad_multi: the UNMODIFIED kernel (fused_sets_kernel: the five-stream fused kernel with the stream-target
head over a table of point sets) compiled for x86 against the SIMT emulator, on the set shapes of the plate's pre-training losses, against
the float64 oracle and against the same call on the two-kernel path.

Bounds.  Loss sums: 3e-6 on both paths (fp32 sums of split-precision products: the bound tests/test_emulated_kernels.py holds the plate's
fused head to).  Gradient: 2e-6 on the two-kernel path (everything split; the bound of test_emulated_plate_entry_points); 1e-4 on the fused
path -- the narrow register-state layouts park fp16 high parts of the states, a 2^-12 = 2.4e-4 rounding per state element that averages
over the ~170 points of a call to ~2e-5, held with the 5x headroom test_emulated_plate_fused gives the same layout at ~100 points."""
import os
import subprocess

import numpy as np
import pytest

from tests import _stream_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = "f16x3"
FLAG_TWO_KERNEL = 0x400


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, capture_output=True)
    from pinn_elastodynamics_amd.capi import PinnLib
    lib = PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))
    lib.set_fused(True)
    return lib


def aligned(nbytes):
    raw = np.zeros(nbytes + 256, dtype=np.uint8)
    off = (-raw.ctypes.data) % 256
    return raw[off:off + nbytes]


def call(emu, flat, layers, sets, mode, ws, wsb, poison=False, grad0=None, keep=None):
    """one library call on host arrays; returns (sums [m, 5], grad)"""
    p32 = flat.astype(np.float32)
    keep = [] if keep is None else keep
    loss = np.full((len(sets), 8), np.nan, np.float32)
    grad = np.full(p32.size, np.nan, np.float32) if grad0 is None else grad0.astype(np.float32).copy()
    rows = []
    for k, (X, tg, w) in enumerate(sets):
        xyz = [np.ascontiguousarray(X[:, j], dtype=np.float32) for j in range(3)]
        t32 = S.device_targets(tg, w, poison)
        keep += xyz + [t32]
        rows.append((xyz[0].ctypes.data if X.shape[0] else 0, xyz[1].ctypes.data if X.shape[0] else 0, xyz[2].ctypes.data if X.shape[0] else 0,
                     X.shape[0], 0 if t32 is None else t32.ctypes.data, w, loss[k].ctypes.data))
    emu.stream_loss_grad_multi(p32.ctypes.data, layers, rows, S.LBP, S.UBP, False, grad.ctypes.data, grad0 is not None, mode, ws.ctypes.data, wsb)
    return loss[:, :S.NOUT].astype(np.float64), grad.astype(np.float64)


CASES = [("part", S.PART_PATTERNS, (50, 33, 17, 64, 1)),          # ragged: no size a multiple of the 64-point step but one
         ("part-empty", S.PART_PATTERNS, (40, 0, 65, 16, 30)),    # an empty set in the middle
         ("dist", S.DIST_PATTERNS, (130, 47)),
         ("dist-empty-first", S.DIST_PATTERNS, (0, 70))]


@pytest.mark.parametrize("name,patterns,sizes", CASES, ids=[c[0] for c in CASES])
def test_stream_sets_emulated(emu, name, patterns, sizes):
    layers = [3, 20, 20, 20, 20, 5]
    rng = np.random.default_rng(11)
    flat = S.fresh_net(layers, rng)
    sets = S.make_sets(patterns, sizes, rng)
    sums, g, _ = S.oracle_sets(flat, layers, sets)
    wsb = emu.workspace_bytes(layers, max(sizes), PREC)
    ws = aligned(wsb)
    assert emu.path_for(layers, PREC, "stream_sets", wsb) == "fused-registers"
    emu.path_counts(reset=True)
    # targets poisoned with NaN in every row of weight 0: they must not reach the result
    f_sums, f_grad = call(emu, flat, layers, sets, PREC, ws, wsb, poison=True)
    cnt = emu.path_counts(reset=True)
    assert cnt["fused-registers"] == 1 and cnt["two-kernel"] == 0, cnt
    t_sums, t_grad = call(emu, flat, layers, sets, emu_mode(PREC) | FLAG_TWO_KERNEL, ws, wsb)
    cnt = emu.path_counts(reset=True)
    assert cnt["two-kernel"] == sum(1 for n in sizes if n > 0) and cnt["fused-registers"] == 0, cnt
    e = dict(fused_loss=S.rel(f_sums, sums), fused_grad=S.rel(f_grad, g), two_loss=S.rel(t_sums, sums), two_grad=S.rel(t_grad, g),
             fused_vs_two=S.rel(f_grad, t_grad))
    print(name, {k: f"{v:.2e}" for k, v in e.items()})
    for k, n in enumerate(sizes):
        if n == 0:
            assert np.all(f_sums[k] == 0) and np.all(t_sums[k] == 0)
    assert np.isfinite(f_grad).all() and np.isfinite(f_sums).all()
    assert e["fused_loss"] < 3e-6 and e["two_loss"] < 3e-6
    assert e["two_grad"] < 2e-6
    assert e["fused_grad"] < 1e-4 and e["fused_vs_two"] < 1e-4


def emu_mode(prec):
    from pinn_elastodynamics_amd.capi import PREC as P
    return P[prec]


def test_stream_sets_accumulate_emulated(emu):
    """accumulate: the gradient adds to what was there, on both paths; without it the old content is overwritten"""
    layers = [3, 20, 20, 20, 20, 5]
    rng = np.random.default_rng(12)
    flat = S.fresh_net(layers, rng)
    sets = S.make_sets(S.DIST_PATTERNS, (70, 20), rng)
    _, g, _ = S.oracle_sets(flat, layers, sets)
    wsb = emu.workspace_bytes(layers, 70, PREC)
    ws = aligned(wsb)
    base = rng.standard_normal(flat.size)
    for mode, tol in ((emu_mode(PREC), 1e-4), (emu_mode(PREC) | FLAG_TWO_KERNEL, 2e-6)):
        _, plain = call(emu, flat, layers, sets, mode, ws, wsb)
        _, acc = call(emu, flat, layers, sets, mode, ws, wsb, grad0=base)
        assert S.rel(plain, g) < tol
        # fp32 addition of the same reduction onto the old content
        assert np.allclose(acc, base.astype(np.float32).astype(np.float64) + plain, rtol=0, atol=4e-7 * np.abs(base).max() + 4e-7 * np.abs(plain).max())


def test_stream_sets_several_steps_per_workgroup_emulated(emu):
    """A grid smaller than the number of steps (pinn_debug_set_fused_grid_cap): a workgroup walks through several sets, its per-set sums
    are flushed as the set changes, and the weight-gradient accumulators persist across the sets."""
    layers = [3] + 4 * [50] + [5]               # padded width 64
    rng = np.random.default_rng(13)
    flat = S.fresh_net(layers, rng)
    sizes = (130, 64, 70, 1, 65)
    sets = S.make_sets(S.PART_PATTERNS, sizes, rng)
    sums, g, _ = S.oracle_sets(flat, layers, sets)
    wsb = emu.workspace_bytes(layers, max(sizes), PREC)
    ws = aligned(wsb)
    emu.lib.pinn_debug_set_fused_grid_cap.argtypes = [__import__("ctypes").c_int]
    old = emu.lib.pinn_debug_set_fused_grid_cap(2)
    try:
        emu.path_counts(reset=True)
        f_sums, f_grad = call(emu, flat, layers, sets, PREC, ws, wsb, poison=True)
        assert emu.path_counts(reset=True)["fused-registers"] == 1
    finally:
        emu.lib.pinn_debug_set_fused_grid_cap(old)
    print("capped grid", f"{S.rel(f_sums, sums):.2e}", f"{S.rel(f_grad, g):.2e}")
    assert S.rel(f_sums, sums) < 3e-6 and S.rel(f_grad, g) < 1e-4


def test_stream_sets_other_depth_falls_back_emulated(emu):
    """3 hidden layers: no fused instantiation -- the sets run one by one on the two-kernel path, same quantities, same normalisation"""
    layers = [3, 20, 20, 20, 5]
    rng = np.random.default_rng(14)
    flat = S.fresh_net(layers, rng)
    sets = S.make_sets(S.DIST_PATTERNS, (40, 90), rng)
    sums, g, _ = S.oracle_sets(flat, layers, sets)
    wsb = emu.workspace_bytes(layers, 90, PREC)
    ws = aligned(wsb)
    assert emu.path_for(layers, PREC, "stream_sets", wsb) == "two-kernel"
    emu.path_counts(reset=True)
    t_sums, t_grad = call(emu, flat, layers, sets, PREC, ws, wsb)
    cnt = emu.path_counts(reset=True)
    assert cnt["two-kernel"] == 2 and cnt["fused-registers"] == 0
    assert S.rel(t_sums, sums) < 3e-6 and S.rel(t_grad, g) < 2e-6
