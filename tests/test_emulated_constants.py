"""CPU: every physics head and kernel path on the host SIMT emulator at material constants and domains where no two quantities
coincide (tests/_general_constants.py).  At the reference's constants c2 == G == rho == 1 and the older tests' domains have equal x and y
spans, so a head that reads c2 for G, drops rho, or a kernel that maps y with x's scale, computes the numbers those tests expect.
Each case also compares the gradient of every residual term on its own (one-hot term weights) with the float64 oracle's."""
import numpy as np
import pytest

from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests._general_constants import CONSTS, LB2, LB3, UB2, UB3, check_terms, rel
from tests.test_emulated_kernels import _step_case, aligned, emu  # noqa: F401  (emu: the module-scoped library fixture)

PLATE_A = (7.3, 0.31, 1.7)        # the plate head is plane stress: set A's E / nu / rho
LBP, UBP = [0.0, 0.1, 0.0], [0.5, 0.4, 10.0]


def net(depth, width, nin=3, nout=7):
    return [nin] + depth * [width] + [nout]


def params(layers, rng, bscale=0.3):
    Ws, bs = po.xavier_init(layers, rng)
    return po.pack_params(Ws, [bscale * rng.standard_normal(b.shape) for b in bs])


def box(n, lb, ub, rng):
    return np.asarray(lb) + (np.asarray(ub) - np.asarray(lb)) * rng.random((n, len(lb)))


def counted(emu, path, fn):
    """run fn() and assert that exactly one library call ran, on ``path``"""
    emu.path_counts(reset=True)
    out = fn()
    pc = emu.path_counts(reset=True)
    assert pc[path] == 1 and sum(pc.values()) == 1, (path, pc)
    return out


# (layers, points, mode, path, gradient bar of the path at the default constants)
WAVE_PATHS = {
    "two-kernel": (net(4, 32), 100, "f16x3", "two-kernel", 2e-6),          # test_wave_loss_grad_emulated
    "fused-registers": (net(4, 32), 100, "f16x3", "fused-registers", 1e-4),  # test_fused_kernel_emulated
    "fused-registers-8x64": (net(8, 64), 40, "f16x3", "fused-registers", 1e-4),
    "fused-lds": (net(8, 80), 17, "f16x3", "fused-lds", 3e-6),              # test_fused_wide_emulated
    "width160": (net(6, 140), 17, "f16x3", "fused-lds", 3e-6),              # test_fused_width160_emulated
    "fp32": (net(3, 20), 100, "fp32", "fp32", 5e-6),                         # test_fp32_mode_emulated
}


@pytest.mark.parametrize("name,cs,plane_strain,per_term", [
    ("two-kernel", "A", 1, True), ("two-kernel", "A", 0, True), ("two-kernel", "B", 1, True), ("two-kernel", "B", 0, False),
    ("fused-registers", "A", 1, True), ("fused-registers", "A", 0, True), ("fused-registers", "B", 1, True), ("fused-registers", "B", 0, False),
    ("fused-registers-8x64", "A", 0, False), ("fused-registers-8x64", "B", 1, False),
    ("fused-lds", "A", 1, True), ("fused-lds", "B", 0, False),
    ("width160", "A", 0, False), ("width160", "B", 1, False),
    ("fp32", "A", 1, True), ("fp32", "A", 0, True), ("fp32", "B", 1, True), ("fp32", "B", 0, True),
])
def test_wave_head_general_constants_emulated(emu, name, cs, plane_strain, per_term):
    """pinn_wave2d_loss_grad on every path, both Hooke laws, on the anisotropic domain: loss sums and gradient (per term) vs the oracle"""
    layers, n, prec, path, tol = WAVE_PATHS[name]
    E, mu, rho = CONSTS[cs]
    rng = np.random.default_rng(41)
    flat = params(layers, rng)
    X = box(n, LB2, UB2, rng)
    p32 = flat.astype(np.float32)
    x, y, t = (np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(3))
    wsb = emu.workspace_bytes(layers, n, prec)
    ws = aligned(wsb)

    def call(tw):
        loss, grad = np.full(8, np.nan, np.float32), np.full(p32.size, np.nan, np.float32)
        counted(emu, path, lambda: emu.wave2d_loss_grad(p32.ctypes.data, layers, x.ctypes.data, y.ctypes.data, t.ctypes.data, n, LB2, UB2, True,
                                                        E, mu, rho, plane_strain, tw, loss.ctypes.data, grad.ctypes.data, False, prec,
                                                        ws.ctypes.data, wsb))
        return loss[:7].copy(), grad

    def oracle(tw):
        ss, g, _ = po.wave2d_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], LB2, UB2, True, E, mu, rho, bool(plane_strain), term_weights=tw)
        return ss, g

    tol_loss = 5e-6 if prec == "fp32" else 2e-6
    if name == "fused-registers-8x64" and cs == "B":
        # measured: loss sums 2.2e-6 here (f_s22 alone 8e-6; the two-kernel path 3e-7, a float32 oracle 1e-7): the 8-layer register-state
        # kernel's tangents carry ~10x the two-kernel path's rounding, and c1 = 102 multiplies it into the constitutive residuals
        tol_loss = 5e-6
    emu.set_fused(path != "two-kernel")
    try:
        check_terms(call, oracle, np.array([1, 2, 3, 1, 0.5, 1, 2.0]) / n, tol_loss, tol, per_term)
    finally:
        emu.set_fused(1)


# (layers, points, mode, path, gradient bar) -- test_emulated_plate_fused / test_emulated_plate_entry_points / test_fp32_mode_plate_and_nc3d_emulated
PLATE_PATHS = {
    "fused-registers": ([3] + 4 * [24] + [5], 70, "f16x3", "fused-registers", 1e-4),
    "fused-lds": ([3] + 8 * [70] + [5], 33, "f16x3", "fused-lds", 2e-6),
    "two-kernel": ([3, 20, 20, 20, 5], 50, "f16x3", "two-kernel", 2e-6),
    "fp32": ([3] + 3 * [24] + [5], 100, "fp32", "fp32", 5e-6),
}


@pytest.mark.parametrize("name,per_term", [("fused-registers", True), ("fused-lds", False), ("two-kernel", True), ("fp32", True)])
def test_plate_head_general_constants_emulated(emu, name, per_term):
    """pinn_plate2d_loss_grad (five streams, composite head, plane stress) at E 7.3 / nu 0.31 / rho 1.7, per term, vs the oracle"""
    lN, n, prec, path, tol = PLATE_PATHS[name]
    E, mu, rho = PLATE_A
    rng = np.random.default_rng(43)
    lD = [3, 10, 10, 5]
    fN, fD, fP = params(lN, rng, 0.2), params(lD, rng, 0.2), params(lD, rng, 0.2)
    C = box(n, LBP, UBP, rng)
    x, y, t = (np.ascontiguousarray(C[:, k], dtype=np.float32) for k in range(3))
    Dref, Pref = pl.net_streams(fD, lD, *C.T), pl.net_streams(fP, lD, *C.T)
    frozen = np.ascontiguousarray(np.stack([Dref, Pref]).astype(np.float32))
    pN = fN.astype(np.float32)
    wsb = emu.workspace_bytes(lN, n, prec)
    ws = aligned(wsb)

    def call(tw):
        loss, grad = np.full(8, np.nan, np.float32), np.full(pN.size, np.nan, np.float32)
        counted(emu, path, lambda: emu.plate2d_loss_grad(pN.ctypes.data, lN, x.ctypes.data, y.ctypes.data, t.ctypes.data, n, LBP, UBP, False,
                                                         frozen.ctypes.data, E, mu, rho, tw, loss.ctypes.data, grad.ctypes.data, False, prec,
                                                         ws.ctypes.data, wsb))
        return loss[:5].copy(), grad

    def oracle(tw):
        ss, g, _ = pl.plate_loss_grad(fN, lN, *C.T, Dref, Pref, E, mu, rho, term_weights=tw)
        return ss, g

    emu.set_fused(path != "two-kernel")
    try:
        check_terms(call, oracle, np.array([10, 7, 13, 9, 11.0]) / n, 5e-6 if prec == "fp32" else 3e-6, tol, per_term)
    finally:
        emu.set_fused(1)


# (layers, points, mode, path, gradient bar) -- test_fused_nc3d_emulated / test_nc3d_entry_points_emulated / test_fp32_mode_plate_and_nc3d_emulated
NC3D_PATHS = {
    "fused-lds": (net(10, 100, 4, 12), 20, "f16x3", "fused-lds", 5e-6),
    "two-kernel": (net(2, 32, 4, 12), 45, "f16x3", "two-kernel", 2e-6),
    "fp32": (net(3, 24, 4, 12), 100, "fp32", "fp32", 5e-6),
}


@pytest.mark.parametrize("name,cs,per_term", [("fused-lds", "A", False), ("two-kernel", "A", True), ("two-kernel", "B", False),
                                              ("fp32", "A", True), ("fp32", "B", True)])
def test_nc3d_head_general_constants_emulated(emu, name, cs, per_term):
    """pinn_nc3d_loss_grad on the anisotropic 3-D domain (spans 30 / 12 / 17 / 9) at sets A and B, per term, vs the oracle"""
    layers, n, prec, path, tol = NC3D_PATHS[name]
    E, mu, rho = CONSTS[cs]
    rng = np.random.default_rng(47)
    flat = params(layers, rng, 0.2)
    X = n3.halfspace_points(n, LB3, UB3, rng)
    p32 = flat.astype(np.float32)
    cols = [np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(4)]
    ptr = [c.ctypes.data for c in cols]
    wsb = emu.workspace_bytes(layers, n, prec)
    ws = aligned(wsb)

    def call(tw):
        loss, grad = np.full(16, np.nan, np.float32), np.full(p32.size, np.nan, np.float32)
        counted(emu, path, lambda: emu.nc3d_loss_grad(p32.ctypes.data, layers, *ptr, n, LB3, UB3, True, E, mu, rho, tw, loss.ctypes.data,
                                                      grad.ctypes.data, False, prec, ws.ctypes.data, wsb))
        return loss[:12].copy(), grad

    def oracle(tw):
        ss, g, _ = n3.nc3d_loss_grad(flat, layers, *X.T, LB3, UB3, True, E, mu, rho, term_weights=tw)
        return ss, g

    emu.set_fused(path != "two-kernel")
    try:
        check_terms(call, oracle, (0.5 + np.random.default_rng(5).random(12)) / n, 5e-6 if prec == "fp32" else 2e-6, tol, per_term)
    finally:
        emu.set_fused(1)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
def test_fields_on_anisotropic_domains_emulated(emu, prec):
    """pinn_wave2d_fields / pinn_nc3d_fields: value and first derivatives on domains with a different span and offset per input -- the input
    map (sx, ox per input) and the first layer's tangent seeds (sx[s] * W[s]) alone, the constants play no part"""
    tol = 5e-6 if prec == "fp32" else 2e-6
    rng = np.random.default_rng(53)
    layers, n = net(3, 32), 90
    flat = params(layers, rng)
    X = box(n, LB2, UB2, rng)
    p32 = flat.astype(np.float32)
    x, y, t = (np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(3))
    wsb = emu.workspace_bytes(layers, n, prec)
    ws = aligned(wsb)
    fo = np.full((28, n), np.nan, np.float32)
    emu.wave2d_fields(p32.ctypes.data, layers, x.ctypes.data, y.ctypes.data, t.ctypes.data, n, LB2, UB2, True, fo.ctypes.data, prec, ws.ctypes.data, wsb)
    out = po.wave2d_fields(flat, layers, *X.T, LB2, UB2, True)
    for k, ref in enumerate([out["Y"]] + out["dY"]):
        assert rel(fo[7 * k:7 * k + 7], ref.T) < tol, (k, rel(fo[7 * k:7 * k + 7], ref.T))
    layers, n = net(2, 48, 4, 12), 60
    flat = params(layers, rng)
    X = n3.halfspace_points(n, LB3, UB3, rng)
    p32 = flat.astype(np.float32)
    cols = [np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(4)]
    wsb = emu.workspace_bytes(layers, n, prec)
    ws = aligned(wsb)
    f3 = np.full((5, 12, n), np.nan, np.float32)
    emu.nc3d_fields(p32.ctypes.data, layers, *[c.ctypes.data for c in cols], n, LB3, UB3, True, f3.ctypes.data, prec, ws.ctypes.data, wsb)
    ref = n3.nc3d_fields(flat, layers, *X.T, LB3, UB3, True)
    for k, r in enumerate([ref["Y"]] + ref["dY"]):
        assert rel(f3[k].T, r) < tol, (k, rel(f3[k].T, r))


@pytest.mark.parametrize("layers,n,n_side", [(net(4, 32), 300, (70, 50))])
def test_step_call_is_the_separate_calls_bit_for_bit_general_constants_emulated(emu, layers, n, n_side):
    """pinn_wave2d_step at set A on the anisotropic domain: the same bits as the separate calls, and the oracle's numbers at set A"""
    E, mu, rho = CONSTS["A"]
    out, (flat, X, tw, sets_np) = _step_case(emu, layers, n, n_side, "f16x3", 7, True, consts=(E, mu, rho), lb=LB2, ub=UB2)
    a, b = out["step"], out["calls"]
    path = "fused-registers" if layers[1] <= 64 else "fused-lds"
    assert a["counts"][path] == 2 and b["counts"][path] == 2 and sum(a["counts"].values()) == 2, (a["counts"], b["counts"])
    for key in ("loss", "grad", "theta", "m", "v"):
        assert np.array_equal(a[key], b[key]), key
    for sa, sb in zip(a["side"], b["side"]):
        assert np.array_equal(sa, sb)
    f64 = flat.astype(np.float64)
    ss, g, _ = po.wave2d_loss_grad(f64, layers, *X.T, LB2, UB2, True, E, mu, rho, term_weights=tw)
    for sx, sy, st, tg, ow, lo in sets_np:
        g += po.data_loss_grad(f64, layers, sx, sy, st, LB2, UB2, True, None if tg is None else tg.T.astype(np.float64), np.asarray(ow))[1]
    assert rel(a["loss"], ss) < 2e-6 and rel(a["grad"], g) < 1e-4


def test_plate_step_call_is_the_separate_calls_bit_for_bit_general_constants_emulated(emu):
    """pinn_plate2d_step at E 7.3 / nu 0.31 / rho 1.7: the same bits as pinn_plate2d_loss_grad + pinn_plate2d_traction_loss_grad +
    pinn_adam_step, and the oracle's numbers at those constants"""
    E, mu, rho = PLATE_A
    lN, n, nh, prec = [3] + 4 * [32] + [5], 200, 40, "f16x3"
    lD = [3, 10, 10, 5]
    rng = np.random.default_rng(59)
    fN, fD, fP = params(lN, rng, 0.2), params(lD, rng, 0.2), params(lD, rng, 0.2)
    X = box(n, LBP, UBP, rng)
    th = rng.random(nh) * np.pi / 2
    H = np.stack([0.1 * np.cos(th), 0.1 * np.sin(th), rng.random(nh) * 10], 1)
    frozen = np.ascontiguousarray(np.stack([pl.net_streams(f, lD, *X.T) for f in (fD, fP)]).astype(np.float32))
    DH, PH = pl.net_streams(fD, lD, *H.T)[0], pl.net_streams(fP, lD, *H.T)[0]
    aux = np.ascontiguousarray(np.concatenate([DH, PH, (-H[:, 0] / 0.1)[None], (-H[:, 1] / 0.1)[None]]).astype(np.float32))
    x, y, t = (np.ascontiguousarray(X[:, k], dtype=np.float32) for k in range(3))
    hx, hy, ht = (np.ascontiguousarray(H[:, k], dtype=np.float32) for k in range(3))
    tw, hw = [10.0 / n, 7.0 / n, 13.0 / n, 9.0 / n, 11.0 / n], [10.0 / nh] * 2
    wsb = emu.workspace_bytes(lN, 1 << 12, prec)
    emu.set_fused(True)
    out = {}
    for mode in ("step", "calls"):
        ws = aligned(wsb)
        theta = fN.astype(np.float32)
        m1, v1 = np.full(theta.size, 0.01, np.float32), np.full(theta.size, 0.02, np.float32)
        loss, hloss, grad = np.full(8, np.nan, np.float32), np.full(8, np.nan, np.float32), np.full(theta.size, np.nan, np.float32)
        emu.path_counts(reset=True)
        if mode == "step":
            emu.plate2d_step(theta.ctypes.data, lN, x.ctypes.data, y.ctypes.data, t.ctypes.data, n, LBP, UBP, False, frozen.ctypes.data, E, mu, rho, tw,
                             loss.ctypes.data, hx.ctypes.data, hy.ctypes.data, ht.ctypes.data, nh, aux.ctypes.data, hw, hloss.ctypes.data, grad.ctypes.data,
                             False, (m1.ctypes.data, v1.ctypes.data, 1e-3, 0.9, 0.999, 1e-8, 2), prec, ws.ctypes.data, wsb)
        else:
            emu.plate2d_loss_grad(theta.ctypes.data, lN, x.ctypes.data, y.ctypes.data, t.ctypes.data, n, LBP, UBP, False, frozen.ctypes.data, E, mu, rho,
                                  tw, loss.ctypes.data, grad.ctypes.data, False, prec, ws.ctypes.data, wsb)
            emu.plate2d_traction_loss_grad(theta.ctypes.data, lN, hx.ctypes.data, hy.ctypes.data, ht.ctypes.data, nh, LBP, UBP, False, aux.ctypes.data, hw,
                                           hloss.ctypes.data, grad.ctypes.data, True, prec, ws.ctypes.data, wsb)
            emu.adam_step(theta.ctypes.data, m1.ctypes.data, v1.ctypes.data, grad.ctypes.data, theta.size, 1e-3, 2)
        out[mode] = dict(theta=theta, m=m1, v=v1, loss=loss[:5].copy(), hloss=hloss[:2].copy(), grad=grad, counts=emu.path_counts(reset=True))
    a, b = out["step"], out["calls"]
    assert a["counts"]["fused-registers"] == 2 and b["counts"]["fused-registers"] == 2 and sum(a["counts"].values()) == 2, (a["counts"], b["counts"])
    for key in ("loss", "hloss", "grad", "theta", "m", "v"):
        assert np.array_equal(a[key], b[key]), key
    ss, g = pl.plate_loss_grad(fN, lN, *X.T, frozen[0].astype(np.float64), frozen[1].astype(np.float64), E, mu, rho, term_weights=np.asarray(tw))[:2]
    ssh, gh = pl.traction_loss_grad(fN, lN, *H.T, DH, PH, weight=10.0 / nh)
    assert rel(a["loss"], ss) < 5e-6 and rel(a["hloss"], ssh) < 5e-6 and rel(a["grad"], g + gh) < 3e-4
