"""CPU tests pinning the oracle: two independent differentiation routes, the
reference's committed weights as known-answer inputs, the committed golden vectors, the FEM bands,
and the TF1 Adam rule."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from oracle.tf1_shaped import MinimalWave, TF1ShapedWave
from tests._general_constants import CONSTS, LB2, UB2, distinct

CASES = ["inf20s", "inf10s", "semi16s", "conf14s"]
GOLDEN_CASES = CASES + ["wave64"]      # + the trained 8x64 net of tools/make_trained64.py (not reference data)


def load_case(golden_dir, case):
    w = np.load(f"{golden_dir}/weights_{case}.npz")
    g = np.load(f"{golden_dir}/golden_{case}.npz")
    layers = [int(v) for v in w["layers"]]
    L = len(layers) - 1
    Ws = [w[f"W{i}"].astype(np.float64) for i in range(L)]
    bs = [w[f"b{i}"].astype(np.float64) for i in range(L)]
    return layers, Ws, bs, g


def test_forward_tangent_equals_tf1_shaped_reverse_mode():
    """closed-form forward tangents == 12 reverse passes + double forward, to round-off (SURVEY Appx C: 1e-14)."""
    rng = np.random.default_rng(0)
    layers = [3, 24, 24, 24, 7]
    Ws, bs = po.xavier_init(layers, rng)
    bs = [0.2 * rng.standard_normal(b.shape) for b in bs]
    lb, ub = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
    X = po.collocation_points(257, lb, ub, rng)
    tw = np.array([1.0] * 4 + [3.0] * 3) / 257
    ss, g, f = po.wave2d_loss_grad(po.pack_params(Ws, bs), layers, X[:, 0], X[:, 1], X[:, 2], lb, ub, True, term_weights=tw)
    for cls in (TF1ShapedWave, MinimalWave):
        m = cls(Ws, bs, lb, ub, True)
        l_uv, l_s, gt, ft = m.flat_grad(X, 1.0, 3.0)
        fr = torch.stack([r.reshape(-1) for r in ft], 1).detach().numpy()
        assert abs(float(l_uv) - ss[:4].sum() / 257) < 1e-13 and abs(float(l_s) - ss[4:].sum() / 257) < 1e-13
        assert np.linalg.norm(fr - f) <= 1e-12 * np.linalg.norm(f)
        assert np.linalg.norm(gt.numpy() - g) <= 1e-12 * np.linalg.norm(g)


def test_raw_input_variant_matches_too():
    rng = np.random.default_rng(1)
    layers = [3, 16, 16, 7]
    Ws, bs = po.xavier_init(layers, rng)
    X = -15 + 30 * rng.random((100, 3))
    ss, g, _ = po.wave2d_loss_grad(po.pack_params(Ws, bs), layers, X[:, 0], X[:, 1], X[:, 2], None, None, False,
                                   term_weights=np.ones(7) / 100)
    _, _, gt, _ = TF1ShapedWave(Ws, bs, [0, 0, 0], [1, 1, 1], False).flat_grad(X)
    assert np.linalg.norm(gt.numpy() - g) <= 1e-12 * np.linalg.norm(g)


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_golden_vectors_reproduce(golden_dir, case):
    layers, Ws, bs, g = load_case(golden_dir, case)
    X = g["X"]
    flat = po.pack_params(Ws, bs)
    out = po.wave2d_fields(flat, layers, X[:, 0], X[:, 1], X[:, 2], g["lb"], g["ub"], bool(g["normalize"]))
    np.testing.assert_allclose(out["Y"], g["Y"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(np.stack(out["dY"]), g["dY"], rtol=1e-11, atol=1e-13)
    ss, gr, f = po.wave2d_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], g["lb"], g["ub"], bool(g["normalize"]),
                                    term_weights=np.ones(7) / X.shape[0])
    np.testing.assert_allclose(f, g["f"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ss, g["sumsq"], rtol=1e-10)
    assert np.linalg.norm(gr - g["grad"]) <= 1e-6 * np.linalg.norm(gr)      # golden grad is stored in fp32


@pytest.mark.parametrize("case,bound", [("inf20s", 5e-5), ("semi16s", 1e-5), ("conf14s", 1e-5)])
def test_known_answer_residual_is_small_at_trained_weights(golden_dir, case, bound):
    """The reference's trained nets satisfy the PDE: any sign / coefficient / derivative-pairing error
    in net_f_sig's restatement makes these O(1) instead of ~1e-5 (SURVEY Appx C item 2)."""
    layers, Ws, bs, g = load_case(golden_dir, case)
    n = g["X"].shape[0]
    assert g["sumsq"][:4].sum() / n < bound and g["sumsq"][4:].sum() / n < bound
    # sanity of the test itself: flipping one sign in the momentum residual breaks it by orders of magnitude
    X = g["X"]
    out = po.wave2d_fields(po.pack_params(Ws, bs), layers, X[:, 0], X[:, 1], X[:, 2], g["lb"], g["ub"], bool(g["normalize"]))
    Jx, Jy, Jt = out["dY"]
    wrong = Jx[:, 4] + Jy[:, 6] + 1.0 * Jt[:, 2]
    assert (wrong ** 2).mean() > 100 * bound


@pytest.mark.parametrize("case", ["inf20s", "semi16s", "conf14s"])
def test_fem_sanity_bands(golden_dir, case):
    """rel-L2(PINN vs the reference's FEM frames) stays in the bands measured at survey time; pins
    the normalisation flag, column order, time stamps (k/4 s) and coordinate shifts."""
    layers, Ws, bs, g = load_case(golden_dir, case)
    fem = np.load(f"{golden_dir}/fem_{case}.npz")
    F = fem["fem"].astype(np.float64)
    pred = po.wave2d_fields(po.pack_params(Ws, bs), layers, F[:, 0], F[:, 1], F[:, 2], g["lb"], g["ub"], bool(g["normalize"]))
    nf = len(fem["frames"])
    for i in range(nf):
        sl = slice(600 * i, 600 * (i + 1))
        r_u = np.linalg.norm(pred["u"][sl] - F[sl, 3]) / np.linalg.norm(F[sl, 3])
        assert abs(r_u - fem["rel_l2"][0][i]) < 1e-4            # reproduces the committed number
        assert r_u < 0.30                                       # and stays a few-to-30 % match (SURVEY Appx C)
    assert fem["rel_l2"][0][0] < 0.2


def test_adam_tf1_rule_differs_from_torch_adam_as_documented():
    rng = np.random.default_rng(2)
    th = rng.standard_normal(50)
    m = np.zeros(50)
    v = np.zeros(50)
    tt = torch.tensor(th.copy(), requires_grad=True)
    opt = torch.optim.Adam([tt], lr=1e-2, eps=1e-8)
    for step in range(1, 4):
        g = rng.standard_normal(50)
        th, m, v = po.adam_tf1_step(th, g, m, v, step, 1e-2)
        tt.grad = torch.tensor(g)
        opt.step()
    # same up to the epsilon placement (tiny for O(1) gradients)
    np.testing.assert_allclose(th, tt.detach().numpy(), rtol=1e-4)
    # hand-computed first step
    th1, m1, v1 = po.adam_tf1_step(np.array([1.0]), np.array([0.5]), np.zeros(1), np.zeros(1), 1, 0.1)
    lr_t = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert abs(th1[0] - (1.0 - lr_t * 0.05 / (np.sqrt(0.00025) + 1e-8))) < 1e-15


def test_total_loss_layouts():
    rng = np.random.default_rng(3)
    layers = [3, 8, 7]
    Ws, bs = po.xavier_init(layers, rng)
    flat = po.pack_params(Ws, bs)
    sets = dict(collo=rng.random((40, 3)), IC=rng.random((10, 3)), SRC=rng.random((12, 5)), UP=rng.random((9, 3)), FIX=rng.random((7, 3)))
    t_inf, _ = po.wave_total_loss_grad(flat, layers, sets, [0, 0, 0], [1, 1, 1], True, "infinite")
    t_semi, _ = po.wave_total_loss_grad(flat, layers, sets, [0, 0, 0], [1, 1, 1], True, "semi_infinite")
    t_conf, _ = po.wave_total_loss_grad(flat, layers, sets, [0, 0, 0], [1, 1, 1], True, "confined")
    assert abs(t_inf["loss"] - (t_inf["loss_f_uv"] + t_inf["loss_f_s"] + t_inf["loss_IC"] + t_inf["loss_SRC"])) < 1e-14   # INF:119
    assert abs(t_semi["loss"] - (5 * t_semi["loss_f_uv"] + 5 * t_semi["loss_f_s"] + 2 * t_semi["loss_IC"] + 2 * t_semi["loss_SRC"]
                                 + 2 * t_semi["loss_NB"])) < 1e-13                                                          # SEMI:127
    assert abs(t_conf["loss"] - (5 * t_conf["loss_f_uv"] + 5 * t_conf["loss_f_s"] + t_conf["loss_SRC"] + t_conf["loss_IC"]
                                 + t_conf["loss_FIX"])) < 1e-13                                                             # CONF:156
    # finite-difference check of the total gradient
    _, g = po.wave_total_loss_grad(flat, layers, sets, [0, 0, 0], [1, 1, 1], True, "semi_infinite")
    d = rng.standard_normal(flat.size)
    eps = 1e-6
    lp, _ = po.wave_total_loss_grad(flat + eps * d, layers, sets, [0, 0, 0], [1, 1, 1], True, "semi_infinite")
    lm, _ = po.wave_total_loss_grad(flat - eps * d, layers, sets, [0, 0, 0], [1, 1, 1], True, "semi_infinite")
    assert abs((lp["loss"] - lm["loss"]) / (2 * eps) - g @ d) < 1e-6 * max(1.0, abs(g @ d))


def test_large_golden_points_and_sums_reproduce(golden_dir):
    """golden_<case>_32k.npz holds no points: oracle/golden_points.py regenerates them from a seed.  The float64 oracle on the
    regenerated points reproduces the stored sums bit-for-bit-class (1e-12) and the stored gradient -- pins generator and seed."""
    from oracle import golden_points as gp
    w = np.load(f"{golden_dir}/weights_inf20s.npz")
    g = np.load(f"{golden_dir}/golden_inf20s_32k.npz")
    layers = [int(v) for v in w["layers"]]
    L = len(layers) - 1
    flat = po.pack_params([w[f"W{i}"] for i in range(L)], [w[f"b{i}"] for i in range(L)])
    n = int(g["n"])
    X = gp.wave_points(g["lb"], g["ub"], tuple(g["src"]), n)
    m = 4096                                   # a prefix: the column norms of f over all points are stored as well
    ss, grad, f = po.wave2d_loss_grad(flat, layers, X[:, 0], X[:, 1], X[:, 2], g["lb"], g["ub"], bool(g["normalize"]), term_weights=np.ones(7) / n)
    assert np.allclose(ss, g["sumsq"], rtol=1e-12, atol=0)
    assert np.linalg.norm(grad - g["grad"]) <= 1e-12 * np.linalg.norm(g["grad"])
    assert np.allclose(np.linalg.norm(f, axis=0), g["f_colnorm"], rtol=1e-12)
    assert f[:m].shape == (m, 7)


# ---- the physics heads at general constants (c1, c2, G, rho pairwise distinct; tests/_general_constants.py) ----------------------------
_DIRS_2D = [(1.0, 0.0), (0.6, -0.8), (-0.3, 1.1)]


def _wave_pts(n, seed):
    return LB2 + (np.asarray(UB2) - LB2) * np.random.default_rng(seed).random((n, 3))


def test_general_constant_sets_are_non_degenerate():
    for E, mu, rho in CONSTS.values():
        assert distinct(E, mu, rho, True) and distinct(E, mu, rho, False)


@pytest.mark.parametrize("cs", sorted(CONSTS))
@pytest.mark.parametrize("plane_strain", [True, False])
@pytest.mark.parametrize("kind", ["P", "S"])
def test_plane_waves_2d_are_residual_free(cs, plane_strain, kind):
    """P (speed sqrt(c1/rho)) and S (sqrt(G/rho)) plane waves solve the 2-D head exactly, in several directions, in both laws;
    the plane-stress wave solves the plate's five-stream head too.  Teeth: the S speed in a P wave (the P speed in an S wave), the
    other law's coefficients, or another density leave an O(amplitude) residual."""
    E, mu, rho = CONSTS[cs]
    X = _wave_pts(400, 1)
    c1, c2, G = po.hooke_coeffs(E, mu, plane_strain)
    for k_dir in _DIRS_2D:
        Y, dY = po.plane_wave_2d(kind, X, k_dir, E=E, mu=mu, rho=rho, plane_strain=plane_strain)
        scale = max(np.abs(Y).max(), max(np.abs(d).max() for d in dY))
        f = po.wave2d_residuals(Y, dY, E, mu, rho, plane_strain)
        assert np.abs(f).max() < 1e-13 * scale, (k_dir, np.abs(f).max(0))
        wrong_speed = np.sqrt((G if kind == "P" else c1) / rho)
        Yw, dYw = po.plane_wave_2d(kind, X, k_dir, E=E, mu=mu, rho=rho, plane_strain=plane_strain, speed=wrong_speed)
        assert np.abs(po.wave2d_residuals(Yw, dYw, E, mu, rho, plane_strain)[:, :2]).max() > 1e-2 * scale
        assert np.abs(po.wave2d_residuals(Y, dY, E, mu, 1.3 * rho, plane_strain)[:, :2]).max() > 1e-2 * scale
        if kind == "P":          # (an S wave strains e11 = -e22 and shears: c1 - c2 = 2 G in both laws, it solves both)
            assert np.abs(po.wave2d_residuals(Y, dY, E, mu, rho, not plane_strain)[:, 4:]).max() > 1e-2 * scale
        if plane_strain:
            continue
        F = po.plane_wave_plate(kind, X, k_dir, E=E, mu=mu, rho=rho)
        fp = pl.plate_residuals(F, E, mu, rho)
        assert np.abs(fp).max() < 1e-13 * scale, (k_dir, np.abs(fp).max(0))
        if kind == "P":
            Fs = po.plane_wave_plate(kind, X, k_dir, E=E, mu=mu, rho=rho, plane_strain=True)      # plane-strain c1 into the plane-stress head
            assert np.abs(pl.plate_residuals(Fs, E, mu, rho)).max() > 1e-2 * scale
        assert np.abs(pl.plate_residuals(F, E, mu, 1.3 * rho)[:, :2]).max() > 1e-2 * scale
        Fw = po.plane_wave_plate(kind, X, k_dir, E=E, mu=mu, rho=rho, speed=wrong_speed)
        assert np.abs(pl.plate_residuals(Fw, E, mu, rho)[:, :2]).max() > 1e-2 * scale


@pytest.mark.parametrize("cs", sorted(CONSTS))
def test_2d_adjoints_are_the_transpose_of_the_heads(cs):
    """<g, f(Y + dY) - f(Y)> == <adjoint(g), dY> for the (affine) wave head in both laws and the plate head"""
    E, mu, rho = CONSTS[cs]
    rng = np.random.default_rng(17)
    N = 60
    for ps in (True, False):
        Y, dY = rng.standard_normal((N, 7)), [rng.standard_normal((N, 7)) for _ in range(3)]
        Yp, dYp = rng.standard_normal((N, 7)), [rng.standard_normal((N, 7)) for _ in range(3)]
        g = rng.standard_normal((N, 7))
        lhs = ((po.wave2d_residuals(Y + Yp, [a + b for a, b in zip(dY, dYp)], E, mu, rho, ps) - po.wave2d_residuals(Y, dY, E, mu, rho, ps)) * g).sum()
        Yb, dYb = po.wave2d_residual_adjoint(g, E, mu, rho, ps)
        rhs = (Yb * Yp).sum() + sum((a * b).sum() for a, b in zip(dYb, dYp))
        assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs)), ps
    F, Fp, g = rng.standard_normal((5, 5, N)), rng.standard_normal((5, 5, N)), rng.standard_normal((N, 5))
    lhs = ((pl.plate_residuals(F + Fp, E, mu, rho) - pl.plate_residuals(F, E, mu, rho)) * g).sum()
    rhs = (pl.plate_residual_adjoint(g, E, mu, rho) * Fp).sum()
    assert abs(lhs - rhs) < 1e-12 * max(1.0, abs(lhs))


def test_forward_tangent_equals_tf1_shaped_reverse_mode_general_constants():
    """test_forward_tangent_equals_tf1_shaped_reverse_mode at constant set A on the anisotropic domain: both routes take E, mu, rho"""
    E, mu, rho = CONSTS["A"]
    rng = np.random.default_rng(4)
    layers = [3, 24, 24, 24, 7]
    Ws, bs = po.xavier_init(layers, rng)
    bs = [0.2 * rng.standard_normal(b.shape) for b in bs]
    X = po.collocation_points(257, LB2, UB2, rng, xc=11.0, yc=7.0)
    tw = np.array([1.0] * 4 + [3.0] * 3) / 257
    ss, g, f = po.wave2d_loss_grad(po.pack_params(Ws, bs), layers, X[:, 0], X[:, 1], X[:, 2], LB2, UB2, True, E, mu, rho, term_weights=tw)
    _, g_ref, _ = po.wave2d_loss_grad(po.pack_params(Ws, bs), layers, X[:, 0], X[:, 1], X[:, 2], LB2, UB2, True, term_weights=tw)
    assert np.linalg.norm(g - g_ref) > 0.1 * np.linalg.norm(g)           # the constants matter here
    for cls in (TF1ShapedWave, MinimalWave):
        m = cls(Ws, bs, LB2, UB2, True, E=E, mu=mu, rho=rho)
        l_uv, l_s, gt, ft = m.flat_grad(X, 1.0, 3.0)
        fr = torch.stack([r.reshape(-1) for r in ft], 1).detach().numpy()
        assert abs(float(l_uv) - ss[:4].sum() / 257) < 1e-13 * max(1.0, ss[:4].sum() / 257)
        assert abs(float(l_s) - ss[4:].sum() / 257) < 1e-13 * max(1.0, ss[4:].sum() / 257)
        assert np.linalg.norm(fr - f) <= 1e-12 * np.linalg.norm(f)
        assert np.linalg.norm(gt.numpy() - g) <= 1e-12 * np.linalg.norm(g)
