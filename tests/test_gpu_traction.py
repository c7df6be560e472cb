"""-m gpu: the traction boundary term of the wave family on the device -- HipEngine.wave_traction_loss_grad, wave_step(traction=...),
DeepHPM(TRAC=...) -- against the float64 reference of tests/_traction_cases.py.

Bounds: the data head's own on the device (tests/test_gpu_paths.py::test_each_path_runs_where_path_for_says, tests/test_gpu_parity.py::
test_data_terms): loss sums 2e-5; gradient 2e-4 where the one-stream kernel of padded width <= 64 runs (its states reach the weight gradient
as fp16 high parts), 2e-5 on the wider layouts, 1e-4 for PINN_PREC_FP32.  The chain is the data head's, only the adjoint seed differs.
One case exceeds them: the single point at 8 x 64 measures 2.10e-04 -- and so does the existing data head (output weights on s11, s22, s12)
at the same net, point and targets: 2.10e-04 against its own float64 oracle (one point averages nothing of the 2^-12 state rounding).  It
is allowed twice the data head's measured error, 4.2e-4 (profiles/wave_traction_calls.txt, section 4)."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as po
from tests import _traction_cases as tc
from tests._traction_cases import LB, UB, rel
from tests.test_gpu_parity import engine, to_dev

pytestmark = pytest.mark.gpu

W8x64, W8x80 = [3] + 8 * [64] + [7], [3] + 8 * [80] + [7]
# (net, points, precision, path, gradient bound).  16385 = one point past one full persistent round of 256 workgroups x 64 points;
# 8193 = one point past one round of 256 workgroups x 32 points of the LDS-operand layout
CASES = [(W8x64, 1, "f16x3", "fused-registers", 4.2e-4), (W8x64, 1000, "f16x3", "fused-registers", 2e-4), (W8x64, 16385, "f16x3", "fused-registers", 2e-4),
         (W8x80, 8193, "f16x3", "fused-lds", 2e-5), (W8x64, 1000, "fp32", "fp32", 1e-4)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def references():
    """inputs and float64 reference of every case, computed once"""
    out = {}
    for layers, n, prec, path, _ in CASES:
        rng = np.random.default_rng(8)
        flat = tc.make_net(layers, rng)
        X, aux = tc.make_set(n, rng)
        w = tc.weights_for(n)
        X32 = X.astype(np.float32)
        ss, g, _ = tc.traction_reference(flat, layers, X32[:, 0], X32[:, 1], X32[:, 2], LB, UB, True, aux, w)
        out[(layers[1], n, prec)] = (flat, X32, aux, w, ss, g)
    return out


@pytest.mark.parametrize("layers,n,prec,path,tol_grad", CASES)
def test_engine_against_the_reference(dev, references, layers, n, prec, path, tol_grad):
    flat, X, aux, w, ss, g = references[(layers[1], n, prec)]
    eng = engine(layers, prec, dev, max(n, 1 << 14))
    theta, xs, a = to_dev(flat, dev), [to_dev(X[:, k], dev) for k in range(3)], to_dev(aux, dev)
    eng.lib.path_counts(reset=True)
    loss, grad = eng.wave_traction_loss_grad(theta, *xs, LB, UB, True, a, w)
    torch.cuda.synchronize()
    counts = eng.lib.path_counts(reset=True)
    assert counts[path] == 1 and sum(counts.values()) == 1, counts
    e_loss, e_grad = rel(loss.cpu().numpy(), ss), rel(grad.cpu().numpy(), g)
    print(f"traction {layers[1]} x {len(layers) - 2}, n = {n}, {prec} ({path}): loss {e_loss:.2e}, gradient {e_grad:.2e}")
    assert e_loss < (1e-4 if prec == "fp32" else 2e-5) and e_grad < tol_grad, (e_loss, e_grad)
    # accumulate adds to what is there
    g2 = grad.clone()
    eng.wave_traction_loss_grad(theta, *xs, LB, UB, True, a, w, grad_out=g2, accumulate=True, packed=True)
    assert rel(g2.cpu().numpy(), 2.0 * grad.cpu().numpy().astype(np.float64)) < 1e-6


def _model_sets(n_collo=20000, n_trac=3000, seed=2):
    rng = np.random.default_rng(seed)
    Collo = po.collocation_points(n_collo, LB, UB, rng)
    SRC, IC = po.ricker_source_set(n_pt=40, n_time=31), po.ic_grid(num=41)
    X, aux = tc.make_set(n_trac, rng)
    TRAC = np.concatenate([X, aux.T.astype(np.float64)], 1)
    return Collo, SRC, IC, TRAC


def test_step_with_traction_is_the_separate_calls_bit_for_bit(dev):
    """wave_step(traction=...) (pinn_wave2d_step_traction) as ONE launch -- the traction set as kind 2 in the one-stream part's set table,
    behind IC and SRC -- against the separate calls the entry point makes inside (pinn_debug_set_step_launch(0): collocation call, the same
    table as one multi-set call, Adam) at 8 x 64, 20 000 collocation points + IC + SRC + TRAC: parameters, moments, gradient and sums, bit
    for bit; two fused-registers counts either way.  Against the public calls (step, then the traction call) the gradient agrees to the
    path's accuracy: either is within 2e-4 of the truth."""
    layers = W8x64
    Collo, SRC, IC, TRAC = _model_sets()
    n = Collo.shape[0]
    flat = tc.make_net(layers, np.random.default_rng(5)).astype(np.float32)
    eng = engine(layers, "f16x3", dev, n)
    col = lambda A, k: to_dev(A[:, k], dev)
    x, y, t = (col(Collo, k) for k in range(3))
    tw = (np.array([1, 2, 3, 1, 0.5, 1, 2.0]) / n).tolist()
    src_t = to_dev(np.concatenate([SRC[:, 3:5].T, np.zeros((5, SRC.shape[0]))]), dev)
    tx, ty, tt = (col(TRAC, k) for k in range(3))
    taux = to_dev(TRAC[:, 3:].T, dev)
    wt = tc.weights_for(TRAC.shape[0])
    out = {}
    for mode in ("step", "inside", "calls"):
        theta = to_dev(flat, dev)
        m, v = torch.full_like(theta, 0.01), torch.full_like(theta, 0.02)
        sums = torch.full((4, 8), float("nan"), device=dev)
        grad = torch.full_like(theta, float("nan"))
        side = [(col(IC, 0), col(IC, 1), col(IC, 2), None, [1.0 / IC.shape[0]] * 4 + [0.0] * 3, sums[1]),
                (col(SRC, 0), col(SRC, 1), col(SRC, 2), src_t, [1.0 / SRC.shape[0]] * 2 + [0.0] * 5, sums[2])]
        eng.lib.path_counts(reset=True)
        if mode in ("step", "inside"):
            eng.lib.set_step_launch(mode == "step")
            try:
                eng.wave_step(theta, x, y, t, LB, UB, True, tw, side, grad, sums[0], adam=(m, v, 1e-3, 3), traction=(tx, ty, tt, taux, wt, sums[3]))
            finally:
                eng.lib.set_step_launch(1)
        else:
            eng.wave_step(theta, x, y, t, LB, UB, True, tw, side, grad, sums[0])
            eng.wave_traction_loss_grad(theta, tx, ty, tt, LB, UB, True, taux, wt, grad_out=grad, accumulate=True, loss_out=sums[3], packed=True)
            eng.adam_step(theta, m, v, grad, 1e-3, 3)
        torch.cuda.synchronize()
        out[mode] = (theta.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), grad.cpu().numpy(), sums.cpu().numpy(), eng.lib.path_counts(reset=True))
    for a, b in zip(out["step"][:5], out["inside"][:5]):
        assert np.array_equal(a, b, equal_nan=True)
    assert out["step"][5] == out["inside"][5] and out["step"][5]["fused-registers"] == 2 and sum(out["step"][5].values()) == 2, out["step"][5]
    assert out["calls"][5]["fused-registers"] == 3
    assert rel(out["step"][3], out["calls"][3].astype(np.float64)) < 4e-4 and rel(out["step"][4][:3, :7], out["calls"][4][:3, :7].astype(np.float64)) < 2e-6
    assert np.isfinite(out["step"][3]).all() and not np.array_equal(out["step"][0], flat)
    ss, _, _ = tc.traction_reference(flat, layers, TRAC[:, 0].astype(np.float32), TRAC[:, 1].astype(np.float32), TRAC[:, 2].astype(np.float32), LB, UB, True,
                                     TRAC[:, 3:].T.astype(np.float32), wt)
    assert rel(out["step"][4][3, :2], ss) < 2e-5


def test_model_with_traction_set_against_the_reference_total_and_training(dev):
    """DeepHPM(TRAC=...)._loss_and_grad against the float64 total (the oracle's total of the other sets + the traction reference), one
    wave_step(traction=...) call (one launch: two path counts); then train(iter=5): finite parameters, five entries of trac_rec, the return tuple as ever."""
    from pinn_elastodynamics_amd.elastic_wave import DeepHPM
    layers = W8x64
    Collo, SRC, IC, TRAC = _model_sets(n_collo=20000, n_trac=1500, seed=6)
    n, nt = Collo.shape[0], TRAC.shape[0]
    m = DeepHPM(Collo, SRC, IC, np.zeros((0, 3)), layers, LB, UB, verbose=False, seed=9, TRAC=TRAC, trac_weight=2.0)
    flat = m.theta.cpu().numpy().astype(np.float64)
    terms, g = po.wave_total_loss_grad(flat, layers, dict(collo=Collo, IC=IC, SRC=SRC), LB, UB, True, "infinite")
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    ss, gt, _ = tc.traction_reference(flat, layers, f32(TRAC[:, 0]), f32(TRAC[:, 1]), f32(TRAC[:, 2]), LB, UB, True, f32(TRAC[:, 3:].T), [2.0 / nt] * 2)
    m.engine.lib.path_counts(reset=True)
    m._loss_and_grad(0, n)
    torch.cuda.synchronize()
    counts = m.engine.lib.path_counts(reset=True)
    assert counts["fused-registers"] == 2 and sum(counts.values()) == 2, counts
    P = m.n_params
    tm = m._terms_from_sums(m._buf[P:].cpu().numpy().reshape(6, 8), n)
    total = terms["loss"] + 2.0 * ss.sum() / nt
    e_term, e_total, e_grad = abs(tm["loss_TRAC"] - ss.sum() / nt) / (ss.sum() / nt), abs(tm["loss"] - total) / total, rel(m._buf[:P].cpu().numpy(), g + gt)
    print(f"model with traction set: loss_TRAC {e_term:.2e}, total {e_total:.2e}, gradient {e_grad:.2e}")
    assert e_term < 2e-5 and e_total < 2e-5 and e_grad < 2e-4
    out = m.train(5, 1e-3, 1)
    assert len(out) == 5 and all(len(v) == 5 for v in out) and len(m.trac_rec) == 5
    assert bool(torch.isfinite(m.theta).all()) and all(np.isfinite(v) and v > 0 for v in m.trac_rec)
    assert abs(m.trac_rec[0] - ss.sum() / nt) / (ss.sum() / nt) < 2e-5          # the first recorded value: the term at the initial weights
