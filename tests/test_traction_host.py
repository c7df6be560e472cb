"""CPU tests of the traction boundary set of the wave family above the kernels: the float64 reference of tests/_traction_cases.py against
torch float64 autograd, the point-set builders, DeepHPM(TRAC=...) on the oracle-backed stand-in engine, and a 2-rank gloo run."""
import os
import subprocess
import sys

import numpy as np
import torch

from oracle import pinn_oracle as po
from pinn_elastodynamics_amd import pointsets as ps
from pinn_elastodynamics_amd.elastic_wave import DeepHPM, DeepHPMConfined
from tests import _traction_cases as tc
from tests._oracle_engine import OracleEngine
from tests.test_host_logic import LAYERS, LB, UB, small_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TractionOracleEngine(OracleEngine):
    """the stand-in engine with the traction call (the shared tests/_oracle_engine.py gains nothing)"""

    def for_layers(self, layers):
        return TractionOracleEngine(layers)

    def wave_traction_loss_grad(self, params, x, y, t, lb, ub, normalize, aux, weights, grad_out=None, accumulate=False, loss_out=None, packed=False):
        self.calls.append(("traction", x.numel()))
        ss, g, _ = tc.traction_reference(self._np(params), self.layers, self._np(x), self._np(y), self._np(t), lb, ub, normalize, self._np(aux),
                                         [float(w) for w in weights])
        return self._put(g, ss, 2, grad_out, accumulate, loss_out)


def test_reference_agrees_with_torch_autograd():
    """The reference is the oracle's forward and reverse pass under this head's seed; torch float64 autograd differentiates the loss as
    written, with no seed of ours: agreement <= 1e-10 relative in sums and gradient ([3, 20, 20, 7], n = 40, inputs normalised)."""
    layers, n = [3, 20, 20, 7], 40
    rng = np.random.default_rng(21)
    flat = tc.make_net(layers, rng)
    X, aux = tc.make_set(n, rng)
    aux = aux.astype(np.float64)
    w = tc.weights_for(n)
    ss, g, _ = tc.traction_reference(flat, layers, X[:, 0], X[:, 1], X[:, 2], LB, UB, True, aux, w)
    th = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    lb, ub = torch.tensor(LB, dtype=torch.float64), torch.tensor(UB, dtype=torch.float64)
    h = 2.0 * (torch.tensor(X) - lb) / (ub - lb) - 1.0
    o = 0
    for l in range(len(layers) - 1):
        W = th[o:o + layers[l] * layers[l + 1]].reshape(layers[l], layers[l + 1])
        o += layers[l] * layers[l + 1]
        b = th[o:o + layers[l + 1]]
        o += layers[l + 1]
        h = h @ W + b
        if l < len(layers) - 2:
            h = torch.tanh(h)
    nx, ny, tx, ty = (torch.tensor(a) for a in aux)
    rx = h[:, 4] * nx + h[:, 6] * ny - tx
    ry = h[:, 6] * nx + h[:, 5] * ny - ty
    sx, sy = (rx * rx).sum(), (ry * ry).sum()
    (w[0] * sx + w[1] * sy).backward()
    assert tc.rel(ss, np.array([sx.item(), sy.item()])) <= 1e-10
    assert tc.rel(g, th.grad.numpy()) <= 1e-10
    assert min(ss) > 0.1 * n      # residuals of order one: no term trivially small


def test_circle_and_general_traction_sets():
    T = ps.circle_traction_set(15.0, 9.0, 2.0, 12, 0.5, 20.0, 5)
    assert T.shape == (60, 7)
    np.testing.assert_allclose(np.hypot(T[:, 3], T[:, 4]), 1.0, rtol=0, atol=1e-15)          # unit normals
    np.testing.assert_allclose(np.hypot(T[:, 0] - 15.0, T[:, 1] - 9.0), 2.0, rtol=0, atol=1e-14)
    # out of the solid = into the cavity: the normal points from the boundary point to the centre
    assert np.all((T[:, 0] - 15.0) * T[:, 3] + (T[:, 1] - 9.0) * T[:, 4] < -1.99)
    assert np.all(T[:, 5:] == 0.0)                                                               # traction-free
    assert np.array_equal(T[:12, 2], np.full(12, 0.5)) and np.array_equal(T[-12:, 2], np.full(12, 20.0))      # time slowest
    assert len({(round(a, 12), round(b, 12)) for a, b in T[:12, :2]}) == 12                    # no point twice (end point excluded)
    load = lambda x, y, t: (np.sin(t), 0.25 * x)
    Tl = ps.circle_traction_set(15.0, 9.0, 2.0, 12, 0.5, 20.0, 5, traction=load)
    np.testing.assert_array_equal(Tl[:, :5], T[:, :5])
    np.testing.assert_allclose(Tl[:, 5], np.sin(T[:, 2]))
    np.testing.assert_allclose(Tl[:, 6], 0.25 * T[:, 0])
    # an inclined straight edge with scaled (quadrature-weighted) normals: taken as given
    P = np.stack([np.linspace(0, 3, 4), np.linspace(0, 6, 4)], 1)
    N = np.tile([[-2.0, 1.0]], (4, 1))
    G = ps.traction_set(P, N, [1.0, 2.0, 3.0])
    assert G.shape == (12, 7) and np.array_equal(G[:, 3:5], np.tile(N, (3, 1))) and np.array_equal(G[4:8, :2], P) and np.all(G[4:8, 2] == 2.0)


def _trac_set(n=37, seed=4, cols=7):
    rng = np.random.default_rng(seed)
    X, aux = tc.make_set(n, rng)
    return np.concatenate([X, aux.T.astype(np.float64)], 1)[:, :cols]


def test_model_with_traction_set_terms_total_and_coefficients():
    Collo, SRC, IC, UP = small_sets()
    TRAC = _trac_set()
    n = Collo.shape[0]
    for case, kw in (("infinite", {}), ("semi_infinite", dict(trac_weight=3.5))):
        eng = TractionOracleEngine(LAYERS)
        m = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, case=case, engine=eng, verbose=False, seed=3, TRAC=TRAC, **kw)
        wt = kw.get("trac_weight", {"infinite": 1.0, "semi_infinite": 2.0}[case])
        assert m.layout["TRAC"] == wt and m.SLOTS[-1] == "TRAC" and len(m.SLOTS) == 6
        flat = m.theta.numpy().astype(np.float64)
        terms, grad = po.wave_total_loss_grad(flat, LAYERS, dict(collo=Collo, IC=IC, SRC=SRC, UP=UP, FIX=None), LB, UB, case == "infinite", case)
        ss, gt, _ = tc.traction_reference(flat, LAYERS, TRAC[:, 0], TRAC[:, 1], TRAC[:, 2], LB, UB, case == "infinite", TRAC[:, 3:].T,
                                          [wt / TRAC.shape[0]] * 2)
        loss_trac = ss.sum() / TRAC.shape[0]
        m._loss_and_grad(0, n)
        P = m.n_params
        sums = m._buf[P:].numpy().reshape(6, 8)
        tm = m._terms_from_sums(sums, n)
        assert abs(tm["loss_TRAC"] - loss_trac) <= 1e-5 * loss_trac and loss_trac > 0.1
        assert abs(tm["loss"] - (terms["loss"] + wt * loss_trac)) <= 1e-5 * tm["loss"]
        np.testing.assert_allclose(m._buf[:P].numpy(), grad + gt, rtol=2e-4, atol=1e-7)
        assert abs(float(np.dot(m._loss_coeffs(n), sums.reshape(-1))) - tm["loss"]) <= 1e-6 * tm["loss"]
        assert ("traction", TRAC.shape[0]) in eng.calls
        d = m.getloss_dict()
        assert set(d) == {"loss", "loss_f_uv", "loss_f_s", "loss_IC", "loss_SRC", "loss_NB", "loss_FIX", "loss_TRAC"}
        assert abs(d["loss_TRAC"] - loss_trac) <= 1e-5 * loss_trac and abs(d["loss"] - tm["loss"]) <= 1e-6 * tm["loss"]
        assert len(m.getloss()) == 6 and abs(m.getloss()[0] - tm["loss"]) <= 1e-6 * tm["loss"]      # the tuple stays, the total holds the term


def test_five_column_set_is_traction_free_and_confined_passes_it_through():
    Collo, SRC, IC, UP = small_sets()
    T5, T7 = _trac_set(cols=5), _trac_set()
    T7[:, 5:] = 0.0
    a = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=TractionOracleEngine(LAYERS), verbose=False, seed=3, TRAC=T5)
    b = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=TractionOracleEngine(LAYERS), verbose=False, seed=3, TRAC=T7)
    assert a.getloss_dict() == b.getloss_dict()
    c = DeepHPMConfined(Collo, SRC, IC, UP, None, LAYERS, [3, 30, 5], [3, 20, 5], LB, UB, engine=TractionOracleEngine(LAYERS), verbose=False,
                        TRAC=T5, trac_weight=0.5)
    assert c.layout["TRAC"] == 0.5 and c.getloss_dict()["loss_TRAC"] > 0.0 and len(c.getloss()) == 6


def test_train_records_the_term_and_keeps_its_return_tuple():
    Collo, SRC, IC, UP = small_sets(n=301)
    m = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=TractionOracleEngine(LAYERS), verbose=False, seed=5, TRAC=_trac_set())
    th0 = m.theta.numpy().astype(np.float64).copy()
    out = m.train(2, 1e-3, 3)
    assert len(out) == 5 and all(len(v) == 6 for v in out) and len(m.trac_rec) == 6 and all(v > 0.0 for v in m.trac_rec)
    # the first recorded value is the term at the initial weights
    T = m.TRAC
    ss, _, _ = tc.traction_reference(th0, LAYERS, T[:, 0], T[:, 1], T[:, 2], LB, UB, True, T[:, 3:].T, [1.0, 1.0])
    assert abs(m.trac_rec[0] - ss.sum() / T.shape[0]) <= 1e-5 * m.trac_rec[0]
    r = m.train_bfgs(1, options=dict(maxiter=3, maxfun=5))
    assert r is not None and np.isfinite(m.theta.numpy()).all()


def test_model_without_traction_set_keeps_five_slots():
    Collo, SRC, IC, UP = small_sets()
    m = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=OracleEngine(LAYERS), verbose=False, seed=3)
    assert m.SLOTS == ("collo", "IC", "SRC", "NB", "FIX") and m._buf.numel() == m.n_params + 40 and "TRAC" not in m.layout and m.trac_rec == []
    assert DeepHPM.SLOTS == m.SLOTS
    m.train(1, 1e-3, 1)
    assert m.trac_rec == [] and "loss_TRAC" not in m.getloss_dict()
    m2 = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, engine=OracleEngine(LAYERS), verbose=False, seed=3, TRAC=np.zeros((0, 5)))
    assert len(m2.SLOTS) == 5


def test_data_parallel_two_ranks_match_single(tmp_path):
    """2-rank gloo run (tests/_dp_worker_traction.py): the traction set row-sharded with the global 1 / n, aux alongside; 5 rows over 2
    ranks and a second model whose set has ONE row, so that rank 0's shard is empty and it makes no call for it."""
    out = str(tmp_path / "dp.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29571", os.path.join(ROOT, "tests", "_dp_worker_traction.py"), out], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    from tests._dp_worker_traction import build
    for tag, rows in (("a", 5), ("b", 1)):
        m = build(rows, TractionOracleEngine)
        m._loss_and_grad(0, m._n_collo)
        np.testing.assert_allclose(z["buf_" + tag + "0"], z["buf_" + tag + "1"], rtol=0, atol=0)            # one all-reduce: the same on both ranks
        np.testing.assert_allclose(z["buf_" + tag + "0"][m.n_params:], m._buf[m.n_params:].numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(z["buf_" + tag + "0"][:m.n_params], m._buf[:m.n_params].numpy(), rtol=2e-4, atol=2e-7)
        assert m._buf[m.n_params + 40] > 0.0
    assert list(z["calls_b"]) == [0, 1]      # rank 0 (empty shard of the one-row set) made no traction call, rank 1 made one
