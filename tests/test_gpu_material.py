"""-m gpu: material identification on the device -- HipEngine.material_sums against the formulas in float64 on the library's own fields call
(head rounding only), against the loss call's sums of squares and against the float64 oracle, and DeepHPM.train(identify=...) end to end against
the same model on the oracle-backed stand-in engine.  Cases and references: tests/_material_cases.py (the same as the emulator tests)."""
import numpy as np
import pytest

from tests import _material_cases as MC

pytestmark = pytest.mark.gpu
_ENGINES = {}


def engine(layers, prec="f16x3"):
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    key = (tuple(layers), prec)
    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(list(layers), precision=prec, device=torch.device("cuda:0"), max_points=1 << 13)
    return _ENGINES[key]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda:0")


def primary(name, layers, prec, n):
    """the sums of an engine in the MINIMUM workspace against the formulas on its own fields call; returns (sums, err / bound)"""
    import torch
    from pinn_elastodynamics_amd.hip_engine import HipEngine
    eng = HipEngine(layers, precision=prec, device=torch.device("cuda:0"), workspace_bytes=0)       # (raised to pinn_min_workspace_bytes)
    X = MC.points(n, seed=77)
    th, xs = dev(MC.fresh_net(tuple(layers))), [dev(X[:, k]) for k in range(3)]
    eng.lib.path_counts(reset=True)
    a = eng.material_sums(th, *xs, MC.LB, MC.UB, True)
    b = eng.material_sums(th, *xs, MC.LB, MC.UB, True)
    assert a.dtype == torch.float64 and a.shape == (14,) and not any(eng.lib.path_counts().values())
    assert torch.equal(a, b), "two calls give different bits"
    F = eng.fields(th, *xs, MC.LB, MC.UB, True).cpu().numpy()
    ref, bound, _ = MC.sums_from_fields(F)
    s = a.cpu().numpy()
    err = np.abs(s - ref)
    print(f"{name} n={n}: max err / bound = {float((err / bound).max()):.3f}")
    assert np.isfinite(s).all() and (err <= bound).all(), err / bound
    return s


@pytest.mark.parametrize("n", MC.PRIMARY_N)
@pytest.mark.parametrize("name,layers,prec", MC.PRIMARY_LINES, ids=[l[0] for l in MC.PRIMARY_LINES])
def test_sums_equal_the_formulas_on_the_fields_call(name, layers, prec, n):
    """PRIMARY check (see the emulator test of the same name): bound 8 eps32 S_k; n = 1 and 33 leave one valid point in a tile; no path counter
    moves; two calls give equal bits"""
    primary(name, layers, prec, n)


@pytest.mark.parametrize("name,layers,prec", MC.PRIMARY_LINES[:2], ids=[l[0] for l in MC.PRIMARY_LINES[:2]])
def test_sums_over_several_tiles_per_wave(name, layers, prec):
    """300 001 points: the chain grid caps at 2048 workgroups = 8192 waves of 32-point tiles, so waves walk a second tile beyond 262 144 points --
    the smallest size at which an accumulator that were reset per tile would be caught"""
    primary(name, layers, prec, 300_001)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("net", MC.SECONDARY_NETS)
def test_sums_against_the_float64_oracle(net, prec):
    """SECONDARY check: max_k |sums_k - oracle_k| / S_k over 1000 collocation points, at most 6 x the same metric of the float32 oracle"""
    layers, flat, X, ref, scale, base = MC.secondary_case(net)
    eng = engine(layers, prec)
    s = eng.material_sums(dev(flat), *[dev(X[:, k]) for k in range(3)], MC.LB, MC.UB, True).cpu().numpy()
    got = MC.scaled_error(s, ref, scale)
    print(f"{net} {prec}: {got:.3e} = {got / base:.2f} x fp32 oracle {base:.3e}")
    assert got <= 6.0 * base


@pytest.mark.parametrize("name,layers,prec", MC.PRIMARY_LINES, ids=[l[0] for l in MC.PRIMARY_LINES])
def test_sums_of_squares_agree_with_the_loss_call(name, layers, prec):
    """CONSISTENCY: sums[0:7] against wave_loss_grad's sums on the same arguments (general constants); tolerance: the larger of the primary bound
    and the fp32 rounding of the loss call's own partial sums, n eps32 sums.  The packed call behind the loss call gives the unpacked call's bits."""
    import torch
    n, consts = 2100, MC.CONSTS_GENERAL[0]
    eng = engine(layers, prec)
    X = MC.points(n, seed=77)
    th, xs = dev(MC.fresh_net(tuple(layers))), [dev(X[:, k]) for k in range(3)]
    a = eng.material_sums(th, *xs, MC.LB, MC.UB, True, *consts)
    loss, _ = eng.wave_loss_grad(th, *xs, MC.LB, MC.UB, True, [1.0] * 7, *consts)
    b = eng.material_sums(th, *xs, MC.LB, MC.UB, True, *consts, packed=True)
    assert torch.equal(a, b)
    s, L = a.cpu().numpy(), loss.cpu().numpy().astype(np.float64)
    _, bound, _ = MC.sums_from_fields(eng.fields(th, *xs, MC.LB, MC.UB, True).cpu().numpy(), *consts)
    tol = np.maximum(bound[:7], n * MC.EPS32 * s[:7])
    print(f"{name}: max |sums - loss| / tol = {float((np.abs(s[:7] - L) / tol).max()):.3f}")
    assert (np.abs(s[:7] - L) <= tol).all()


def test_empty_set_and_output_checks():
    import torch
    layers = [3] + 4 * [32] + [7]
    eng = engine(layers)
    th, e = dev(MC.fresh_net(tuple(layers))), torch.empty(0, dtype=torch.float32, device="cuda:0")
    out = torch.full((14,), 7.0, dtype=torch.float64, device="cuda:0")
    assert eng.material_sums(th, e, e, e, MC.LB, MC.UB, True, out=out) is out and not out.cpu().numpy().any()
    with pytest.raises(AssertionError):
        eng.material_sums(th, e, e, e, MC.LB, MC.UB, True, out=torch.zeros(14, dtype=torch.float32, device="cuda:0"))


def test_identified_training_trajectory_matches_oracle_engine():
    """test_gpu_parity.test_training_trajectory_matches_oracle_engine with identify=(E, mu, rho): 3000 collocation points, 4x32, 25 steps, two
    blocks, from E = 3.5, mu = 0.3, rho = 1.2; the GPU model against the same model on OracleMaterialEngine -- losses and each constant's
    trajectory at rtol 2e-3, and the constants have moved"""
    from oracle import pinn_oracle as po
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    layers = [3] + 4 * [32] + [7]
    rng = np.random.default_rng(4)
    Collo = po.collocation_points(3000, MC.LB, MC.UB, rng)
    SRC = po.ricker_source_set(n_pt=20, n_time=30)
    IC = po.ic_grid(num=15)
    UP = np.stack([rng.random(200) * 30, np.full(200, 30.0), rng.random(200) * 20], 1)
    kw = dict(case="infinite", seed=21, verbose=False, E=3.5, mu=0.3, rho=1.2)
    identify = dict(params=("E", "mu", "rho"), lr=1e-2)
    m_gpu = DeepHPM(Collo, SRC, IC, UP, layers, MC.LB, MC.UB, **kw)
    m_ref = DeepHPM(Collo, SRC, IC, UP, layers, MC.LB, MC.UB, engine=MC.OracleMaterialEngine(layers), **kw)
    np.testing.assert_array_equal(m_gpu.theta.cpu().numpy(), m_ref.theta.numpy())
    out_gpu = m_gpu.train(25, 1e-3, 2, identify=identify)
    out_ref = m_ref.train(25, 1e-3, 2, identify=identify)
    for a, b in zip(out_gpu, out_ref):
        np.testing.assert_allclose(np.array(a), np.array(b), rtol=2e-3, atol=1e-7)
    rg, rr = np.array(m_gpu.material_rec), np.array(m_ref.material_rec)
    assert rg.shape == (50, 4) and np.array_equal(rg[:, 0], np.arange(1, 51)) and np.array_equal(rg[:, 0], rr[:, 0])
    for k, name in enumerate(("E", "mu", "rho"), start=1):
        print(f"{name}: {rg[0, k]:.6f} -> {rg[-1, k]:.6f} (stand-in {rr[-1, k]:.6f}), max rel dev {float(np.abs(rg[:, k] / rr[:, k] - 1).max()):.2e}")
        np.testing.assert_allclose(rg[:, k], rr[:, k], rtol=2e-3)
    assert abs(m_gpu.E - 3.5) > 1e-2 and abs(m_gpu.mu - 0.3) > 1e-3 and abs(m_gpu.rho - 1.2) > 1e-2
