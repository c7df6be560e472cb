"""-m gpu: every kernel path and physics head on the device at material constants and domains where no two quantities coincide
(tests/_general_constants.py), each residual term's gradient on its own against the float64 oracle, the path that ran asserted with the
library's counters; the one-call steps at those constants bit for bit against the separate calls; the model class's Adam trajectory at
those constants against the oracle-backed engine's."""
import numpy as np
import pytest
import torch

from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests._general_constants import CONSTS, LB2, LB3, UB2, UB3, check_terms, rel

pytestmark = pytest.mark.gpu

PLATE_A = (7.3, 0.31, 1.7)        # the plate head is plane stress: set A's E / nu / rho
LBP, UBP = [0.0, 0.1, 0.0], [0.5, 0.4, 10.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def net(depth, width, nin=3, nout=7):
    return [nin] + depth * [width] + [nout]


def params(layers, rng, bscale=0.2):
    Ws, bs = po.xavier_init(layers, rng)
    return po.pack_params(Ws, [bscale * rng.standard_normal(b.shape) for b in bs])


def engine(layers, prec, dev, n):
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    return HipEngine(layers, precision=prec, device=dev, max_points=n)


def counted(eng, path, fn):
    eng.lib.path_counts(reset=True)
    out = fn()
    pc = eng.lib.path_counts(reset=True)
    assert pc[path] == 1 and sum(pc.values()) == 1, (path, pc)
    return out


# the rows of test_gpu_paths.test_each_path_runs_where_path_for_says, with that test's bars (loss sums and gradient)
WAVE_ROWS = [(net(8, 64), "f16x3", "fused-registers"), (net(4, 32), "bf16", "fused-registers"), (net(8, 80), "f16x3", "fused-lds"),
             (net(6, 140), "f16x3", "fused-lds"), (net(5, 64), "f16x3", "two-kernel"), (net(4, 80), "f16x3", "two-kernel"),
             (net(8, 64), "fp32", "fp32")]
TOL = {"f16x3": 2e-5, "bf16": 3e-2, "fp32": 1e-4}


@pytest.mark.parametrize("cs,plane_strain", [("A", 1), ("B", 0)])
@pytest.mark.parametrize("layers,prec,expected", WAVE_ROWS)
def test_wave_head_general_constants_on_every_path(dev, layers, prec, expected, cs, plane_strain):
    """pinn_wave2d_loss_grad at set A (plane strain) and set B (plane stress) on the anisotropic domain, 3000 points: loss sums, the full
    gradient and each term's gradient against the oracle; each call counted on the path pinn_path_for names"""
    E, mu, rho = CONSTS[cs]
    n = 3000
    rng = np.random.default_rng(61)
    flat = params(layers, rng)
    X = LB2 + (np.asarray(UB2) - LB2) * rng.random((n, 3))
    eng = engine(layers, prec, dev, n)
    assert eng.path("wave") == expected
    theta = to_dev(flat, dev)
    xs = [to_dev(X[:, k], dev) for k in range(3)]

    def call(tw):
        loss, grad = counted(eng, expected, lambda: eng.wave_loss_grad(theta, *xs, LB2, UB2, True, tw, E, mu, rho, bool(plane_strain)))
        return loss.cpu().numpy()[:7].astype(np.float64), grad.cpu().numpy().astype(np.float64)

    def oracle(tw):
        ss, g, _ = po.wave2d_loss_grad(flat, layers, *X.T, LB2, UB2, True, E, mu, rho, bool(plane_strain), term_weights=tw)
        return ss, g

    check_terms(call, oracle, np.array([1, 2, 3, 1, 0.5, 1, 2.0]) / n, TOL[prec], TOL[prec], tol_sum=TOL[prec])


# (layers, points, path, loss bar, gradient bar): test_gpu_plate's fused / two-kernel cases and the width-96 layout's
PLATE_ROWS = [(net(8, 64, 3, 5), 4096, "fused-registers", 5e-5, 5e-5), (net(8, 70, 3, 5), 4096, "fused-lds", 5e-6, 3e-5),
              ([3, 32, 32, 32, 5], 3000, "two-kernel", 5e-5, 5e-5)]


@pytest.mark.parametrize("lN,n,expected,tol_loss,tol_grad", PLATE_ROWS)
def test_plate_head_general_constants(dev, lN, n, expected, tol_loss, tol_grad):
    """pinn_plate2d_loss_grad (plane stress, composite head) at E 7.3 / nu 0.31 / rho 1.7: per term against the oracle"""
    E, mu, rho = PLATE_A
    rng = np.random.default_rng(67)
    lD = [3, 10, 10, 5]
    fN, fD, fP = params(lN, rng), params(lD, rng), params(lD, rng)
    C = LBP + (np.asarray(UBP) - LBP) * rng.random((n, 3))
    Dref, Pref = pl.net_streams(fD, lD, *C.T), pl.net_streams(fP, lD, *C.T)
    eng = engine(lN, "f16x3", dev, n)
    assert eng.path("plate") == expected
    theta = to_dev(fN, dev)
    xs = [to_dev(C[:, k], dev) for k in range(3)]
    frozen = to_dev(np.stack([Dref, Pref]), dev)

    def call(tw):
        loss, grad = counted(eng, expected, lambda: eng.plate_loss_grad(theta, *xs, LBP, UBP, False, frozen, tw, E, mu, rho))
        return loss.cpu().numpy()[:5].astype(np.float64), grad.cpu().numpy().astype(np.float64)

    def oracle(tw):
        ss, g, _ = pl.plate_loss_grad(fN, lN, *C.T, Dref, Pref, E, mu, rho, term_weights=tw)
        return ss, g

    check_terms(call, oracle, np.array([10, 7, 13, 9, 11.0]) / n, tol_loss, tol_grad, tol_sum=tol_grad)


@pytest.mark.parametrize("cs", sorted(CONSTS))
@pytest.mark.parametrize("layers,n,expected", [(net(10, 128, 4, 12), 1500, "fused-lds"), (net(3, 64, 4, 12), 3000, "two-kernel")])
def test_nc3d_head_general_constants(dev, layers, n, expected, cs):
    """pinn_nc3d_loss_grad on the anisotropic 3-D domain at sets A and B: per term against the oracle (test_gpu_nc3d's bar 2e-5)"""
    E, mu, rho = CONSTS[cs]
    rng = np.random.default_rng(71)
    flat = params(layers, rng)
    X = n3.halfspace_points(n, LB3, UB3, rng)
    eng = engine(layers, "f16x3", dev, n)
    assert eng.path("nc3d") == expected
    theta = to_dev(flat, dev)
    xs = [to_dev(X[:, k], dev) for k in range(4)]

    def call(tw):
        loss, grad = counted(eng, expected, lambda: eng.nc3d_loss_grad(theta, *xs, LB3, UB3, True, tw, E, mu, rho))
        return loss.cpu().numpy()[:12].astype(np.float64), grad.cpu().numpy().astype(np.float64)

    def oracle(tw):
        ss, g, _ = n3.nc3d_loss_grad(flat, layers, *X.T, LB3, UB3, True, E, mu, rho, term_weights=tw)
        return ss, g

    check_terms(call, oracle, (0.5 + np.random.default_rng(5).random(12)) / n, 2e-5, 2e-5, tol_sum=2e-5)


def test_fields_on_anisotropic_domains(dev):
    """wave2d / nc3d fields (value + first derivatives) on domains with their own span and offset per input: the input map and the first
    layer's tangent seeds"""
    rng = np.random.default_rng(73)
    layers, n = net(4, 32), 3000
    flat = params(layers, rng)
    X = LB2 + (np.asarray(UB2) - LB2) * rng.random((n, 3))
    eng = engine(layers, "f16x3", dev, n)
    F = eng.fields(to_dev(flat, dev), *[to_dev(X[:, k], dev) for k in range(3)], LB2, UB2, True).cpu().numpy().reshape(4, 7, n)
    out = po.wave2d_fields(flat, layers, *X.T, LB2, UB2, True)
    for k, ref in enumerate([out["Y"]] + out["dY"]):
        assert rel(F[k].T, ref) < 2e-5, k
    layers = net(10, 128, 4, 12)
    flat = params(layers, rng)
    X = n3.halfspace_points(1500, LB3, UB3, rng)
    eng = engine(layers, "f16x3", dev, 1500)
    F = eng.nc3d_fields(to_dev(flat, dev), *[to_dev(X[:, k], dev) for k in range(4)], LB3, UB3, True).cpu().numpy().reshape(5, 12, 1500)
    ref = n3.nc3d_fields(flat, layers, *X.T, LB3, UB3, True)
    for k, r in enumerate([ref["Y"]] + ref["dY"]):
        assert rel(F[k].T, r) < 2e-5, k


def test_step_call_is_the_separate_calls_bit_for_bit_general_constants(dev):
    """test_gpu_paths.test_step_call_is_the_separate_calls_bit_for_bit_on_the_gpu with the model at set A on the anisotropic domain"""
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    E, mu, rho = CONSTS["A"]
    rng = np.random.default_rng(2)
    Collo = po.collocation_points(30001, LB2, UB2, rng, xc=11.0, yc=7.0)
    SRC, IC = po.ricker_source_set(xc=11.0, yc=7.0, n_pt=40, n_time=31), po.ic_grid(-4.0, 26.0, 3.0, 11.0, num=41)
    out = {}
    for step_call in (True, False):
        m = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), net(8, 64), LB2, UB2, verbose=False, seed=9, step_call=step_call, E=E, mu=mu, rho=rho)
        m.engine.lib.path_counts(reset=True)
        losses = m.train(5, 1e-3, 1)
        out[step_call] = (m.theta.cpu().numpy(), m.adam_m.cpu().numpy(), m.adam_v.cpu().numpy(), np.array(losses), m.engine.lib.path_counts(reset=True))
    for a, b in zip(out[True][:4], out[False][:4]):
        assert np.array_equal(a, b)
    assert out[True][4]["fused-registers"] == out[False][4]["fused-registers"] > 0 and out[True][4]["two-kernel"] == 0


def test_plate_step_call_is_the_separate_calls_bit_for_bit_general_constants(dev):
    """pinn_plate2d_step at E 7.3 / nu 0.31 / rho 1.7 against pinn_plate2d_loss_grad + pinn_plate2d_traction_loss_grad: identical bits"""
    E, mu, rho = PLATE_A
    layers = net(8, 64, 3, 5)
    n, nh = 20000, 3000
    rng = np.random.default_rng(6)
    theta = to_dev(params(layers, rng), dev)
    X = LBP + (np.asarray(UBP) - LBP) * rng.random((n, 3))
    H = po.collocation_points(nh, [0, 0, 0], [0.1, 0.1, 10.0], rng)
    xs = [to_dev(X[:, k], dev) for k in range(3)]
    hs = [to_dev(H[:, k], dev) for k in range(3)]
    frozen = to_dev(0.3 * rng.standard_normal((2, 5, 5, n)), dev)
    aux = to_dev(0.3 * rng.standard_normal((12, nh)), dev)
    eng = engine(layers, "f16x3", dev, 1 << 16)
    tw, hw = [10.0 / n, 7.0 / n, 13.0 / n, 9.0 / n, 11.0 / n], [10.0 / nh] * 2
    g1, l1, h1 = (torch.full((eng.n_params,), float("nan"), device=dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev))
    eng.plate_step(theta, *xs, LBP, UBP, False, frozen, tw, (*hs, aux, hw), g1, l1, h1, E, mu, rho)
    g2, l2, h2 = (torch.full((eng.n_params,), float("nan"), device=dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev))
    eng.plate_loss_grad(theta, *xs, LBP, UBP, False, frozen, tw, E, mu, rho, grad_out=g2, accumulate=False, loss_out=l2)
    eng.traction_loss_grad(theta, *hs, LBP, UBP, False, aux, hw, grad_out=g2, accumulate=True, loss_out=h2, packed=True)
    assert torch.isfinite(g1).all() and torch.equal(g1, g2) and torch.equal(l1[:5], l2[:5]) and torch.equal(h1[:2], h2[:2])
    g3 = torch.zeros_like(g2)
    eng.plate_loss_grad(theta, *xs, LBP, UBP, False, frozen, tw, grad_out=g3, accumulate=False)          # (the constants matter here)
    assert rel(g3.cpu().numpy(), g1.cpu().numpy().astype(np.float64)) > 1e-2


def test_training_trajectory_matches_oracle_engine_general_constants(dev):
    """test_gpu_parity.test_training_trajectory_matches_oracle_engine with the model at set A (E, mu, rho through elastic_wave.py,
    hip_engine.py and capi.py to the kernels) on the anisotropic domain"""
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    from tests._oracle_engine import OracleEngine
    E, mu, rho = CONSTS["A"]
    layers = net(4, 32)
    rng = np.random.default_rng(4)
    Collo = po.collocation_points(3000, LB2, UB2, rng, xc=11.0, yc=7.0)
    SRC = po.ricker_source_set(xc=11.0, yc=7.0, n_pt=20, n_time=30)
    IC = po.ic_grid(-4.0, 26.0, 3.0, 11.0, num=15)
    kw = dict(seed=21, verbose=False, E=E, mu=mu, rho=rho)
    m_gpu = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), layers, LB2, UB2, **kw)
    m_ref = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), layers, LB2, UB2, engine=OracleEngine(layers), **kw)
    np.testing.assert_array_equal(m_gpu.theta.cpu().numpy(), m_ref.theta.numpy())
    out_gpu = m_gpu.train(25, 1e-3, 2)
    out_ref = m_ref.train(25, 1e-3, 2)
    for a, b in zip(out_gpu, out_ref):
        np.testing.assert_allclose(np.array(a), np.array(b), rtol=2e-3, atol=1e-7)
    assert rel(m_gpu.theta.cpu().numpy(), m_ref.theta.numpy()) < 2e-3
    assert out_gpu[4][-1] < out_gpu[4][0]
