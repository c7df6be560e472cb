"""CPU tests of the host side of predict_device / predict_frames / validate / train(validate=...) (no library): a stand-in engine that
evaluates the predict rows and the error sums in numpy (tests/_oracle_engine.OracleEngine plus the two calls), as tests/test_refine_host.py
does for refinement."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from pinn_elastodynamics_amd import pointsets as ps
from pinn_elastodynamics_amd import validate as V
from pinn_elastodynamics_amd.elastic_wave import DeepHPM, DeepHPMConfined
from pinn_elastodynamics_amd.plate_hole import PINN
from tests import _predict_cases as PC
from tests import _refine_cases as RC
from tests._oracle_engine import OracleEngine

LAYERS = [3, 12, 12, 7]


class PredictEngine(OracleEngine):
    """OracleEngine with HipEngine's wave_predict / field_error_sums: the float64 predict rows rounded to fp32, the sums by numpy"""

    def wave_predict(self, params, x, y, t, lb, ub, normalize, out=None, packed=False):
        self.calls.append(("predict", self._np(x), self._np(y), self._np(t)))
        o = po.wave2d_fields(self._np(params), self.layers, self._np(x), self._np(y), self._np(t), lb, ub, normalize)
        return torch.from_numpy(np.stack([o[k] for k in PC.WAVE_ROWS]).astype(np.float32))

    def field_error_sums(self, pred, rows, ref, out=None):
        self.calls.append(("errsums", tuple(int(r) for r in rows), tuple(ref.shape)))
        p, r = pred.numpy().astype(np.float64)[list(rows)], ref.numpy().astype(np.float64)
        return torch.from_numpy(np.stack([((p - r) ** 2).sum(1), (r ** 2).sum(1)]))


def model(cls=DeepHPM, n=60):
    rng = np.random.default_rng(2)
    Collo, SRC, IC, UP = po.collocation_points(n, RC.LB, RC.UB, rng), po.ricker_source_set(n_pt=4, n_time=3), po.ic_grid(num=4), np.zeros((0, 3))
    eng = PredictEngine(LAYERS)
    if cls is DeepHPMConfined:
        return cls(Collo, SRC, IC, UP, None, LAYERS, None, None, RC.LB, RC.UB, engine=eng, verbose=False, seed=3), eng
    return cls(Collo, SRC, IC, UP, LAYERS, RC.LB, RC.UB, engine=eng, verbose=False, seed=3), eng


def test_predict_frames_tiles_space_per_frame_on_the_device():
    m, eng = model()
    x, y, times = np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0]).reshape(-1, 1), np.array([0.5, 7.0])
    out = m.predict_frames(x, y, times)
    calls = [c for c in eng.calls if c[0] == "predict"]
    assert len(calls) == 1                                                   # one predict call for all frames
    _, cx, cy, ct = calls[0]
    assert cx.tolist() == [1, 2, 3, 1, 2, 3] and cy.tolist() == [4, 5, 6, 4, 5, 6] and ct.tolist() == [0.5, 0.5, 0.5, 7, 7, 7]
    assert tuple(out.shape) == (2, 8, 3)
    for k, tk in enumerate(times):
        want = np.concatenate(m.predict(x, y, np.full(3, tk)), axis=1).T      # [8, 3]
        assert np.allclose(out[k].numpy(), want, rtol=1e-5, atol=1e-7)       # (predict forms e12 in fp32 from the fields call; the order is the call record's)
    assert np.array_equal(m.predict_device(x, y, np.full(3, 7.0)).numpy(), out[1].numpy())
    assert tuple(m.predict_device(torch.tensor(x), torch.tensor(x), torch.tensor(x)).shape) == (8, 3)      # device tensors in
    with pytest.raises(ValueError):
        m.predict_device(x, y)


def test_validate_maps_names_to_rows_and_rejects_unknown_names():
    m, eng = model()
    X = RC.points(40, seed=8)
    cols = (X[:, 0:1], X[:, 1:2], X[:, 2:3])
    pred = dict(zip(DeepHPM.PREDICT_FIELDS, m.predict(*cols)))
    rng = np.random.default_rng(1)
    ref = {k: pred[k] + 0.1 * rng.standard_normal(pred[k].shape) for k in ("u", "v", "s11", "s22", "s12", "e12")}
    eng.calls.clear()
    got = m.validate(*cols, ref, fields=("s12", "u", "e12"))
    assert [c[0] for c in eng.calls] == ["predict", "errsums"] and eng.calls[1][1:] == ((4, 0, 7), (3, 40))
    assert list(got) == ["s12", "u", "e12"]
    for k in got:
        assert got[k] == pytest.approx(ps.relative_l2(pred[k], np.asarray(ref[k], dtype=np.float32)), rel=1e-6)
    assert list(m.validate(*cols, ref)) == ["u", "v", "s11", "s22", "s12"]      # the default: what FEM frames carry
    with pytest.raises(ValueError, match="unknown field"):
        m.validate(*cols, ref, fields=("u", "ut"))
    with pytest.raises(ValueError, match="no column"):
        m.validate(*cols, ref, fields=("e11",))
    with pytest.raises(ValueError, match="rows"):
        m.validate(*cols, dict(ref, u=ref["u"][:5]), fields=("u",))


def test_field_names_are_those_of_predicts_tuple_in_every_class():
    assert DeepHPM.PREDICT_FIELDS == PINN.PREDICT_FIELDS == PC.WAVE_ROWS
    assert V.field_rows(list(PINN.PREDICT_FIELDS), PINN.VALIDATE_FIELDS) == [0, 1, 2, 3, 4]
    assert V.field_rows(list(PINN.PREDICT_FIELDS), ("e12", "v")) == [7, 1] and PINN.PREDICT_INPUTS == ("x", "y", "t")


class PlatePredictEngine(PredictEngine):
    """... and HipEngine's plate_predict: the composite rows in float64 from the net's streams and the frozen block handed in"""

    def plate_predict(self, params, x, y, t, lb, ub, normalize, frozen, out=None, packed=False):
        self.calls.append(("predict", self._np(x), self._np(y), self._np(t)))
        N = pl.net_streams(self._np(params), self.layers, self._np(x), self._np(y), self._np(t))
        fr = self._np(frozen)
        F = pl.composite(N, fr[0], fr[1])
        return torch.from_numpy(np.stack([F[0, 0], F[0, 1], F[0, 2], F[0, 3], F[0, 4], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]]).astype(np.float32))

    def net_streams(self, params, x, y, t, lb, ub, normalize):
        self.calls.append(("streams", x.numel()))
        return super().net_streams(params, x, y, t, lb, ub, normalize)


def test_plate_train_validate_holds_the_frozen_streams_once():
    """PINN: predict_device is the composite of predict; train(validate=...) records at the right steps, evaluates the frozen D / P nets at the
    validation points ONCE (two net_streams calls when the schedule is built, none per validation) and makes no extra call when None"""
    from tests.test_plate_host import LB, LD, LN, LP, UB, nets, plate_sets
    _, rng = nets(2)
    eng = {"uv": PlatePredictEngine(LN), "dist": PlatePredictEngine(LD), "part": PlatePredictEngine(LP)}
    m = PINN(*plate_sets(rng), LN, LD, LP, LB, UB, engines=eng, verbose=False, seed=2)
    X = np.stack([rng.random(30) * 0.5, rng.random(30) * 0.5, rng.random(30) * 10], 1)
    cols = (X[:, 0:1], X[:, 1:2], X[:, 2:3])
    host = np.concatenate(m.predict(*cols), axis=1).T
    assert np.allclose(m.predict_device(*cols).numpy(), host, rtol=1e-5, atol=1e-7)
    ref = {k: host[j] + 0.1 for j, k in enumerate(PINN.VALIDATE_FIELDS)}
    calls = lambda kind: [c for e in eng.values() for c in e.calls if c[0] == kind]
    for e in eng.values():
        e.calls.clear()
    m.train(2, 1e-4)
    assert not calls("predict") and not calls("errsums") and not getattr(m, "val_rec", [])
    streams_before = len(calls("streams"))
    m.train(4, 1e-4, validate=dict(every=2, points=cols, ref=ref, fields=("u", "s12")))
    assert [s for s, _ in m.val_rec] == [2, 4] and len(calls("predict")) == 2 and len(calls("errsums")) == 2
    assert len(calls("streams")) - streams_before == 2                          # D and P at the validation points, once
    assert m.val_rec[-1][1] == m.validate(*cols, ref, fields=("u", "s12"))


@pytest.mark.parametrize("cls", [DeepHPM, DeepHPMConfined])
def test_train_validate_records_at_the_right_steps(cls):
    m, eng = model(cls)
    X = RC.points(25, seed=9)
    cols = (X[:, 0:1], X[:, 1:2], X[:, 2:3])
    ref = {k: np.ones((25, 1)) for k in ("u", "v")}
    eng.calls.clear()
    m.train(2, 1e-3, 2)                                                      # validate=None: no predict, no error sums, no record
    assert not [c for c in eng.calls if c[0] in ("predict", "errsums")] and not getattr(m, "val_rec", [])
    base = [c[0] for c in eng.calls]
    eng.calls.clear()
    m.train(3, 1e-3, 2, validate=dict(every=2, points=cols, ref=ref, fields=("u", "v")))       # steps 1..6 over two blocks
    assert [s for s, _ in m.val_rec] == [2, 4, 6] and all(list(d) == ["u", "v"] and np.isfinite(list(d.values())).all() for _, d in m.val_rec)
    extra = [c[0] for c in eng.calls if c[0] in ("predict", "errsums")]
    assert extra == ["predict", "errsums"] * 3
    assert len([c for c in eng.calls if c[0] not in ("predict", "errsums")]) == len(base) * 3 // 2      # the training calls themselves are unchanged
    assert eng.calls[[c[0] for c in eng.calls].index("predict")][1].size == 25                           # the points were uploaded once, as given
    want = m.validate(*cols, ref, fields=("u", "v"))
    assert m.val_rec[-1][1] == want                                          # the last record is the model as train() left it
    with pytest.raises(ValueError, match="missing"):
        m.train(1, 1e-3, 1, validate=dict(every=1, points=cols))
    with pytest.raises(ValueError):
        m.train(1, 1e-3, 1, validate=dict(every=0, points=cols, ref=ref))
