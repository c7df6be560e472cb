"""CPU tests of the host side of refine_collocation in the plate and 3-D classes (no library): bookkeeping, the shard-only rule, the frozen-column
update of PINN, argument checks -- with a stand-in engine that scores and selects in numpy (tests/_oracle_engine.OracleEngine plus the refinement
calls)."""
import numpy as np
import pytest
import torch

from oracle import nc3d_oracle as n3
from oracle import plate_oracle as pl
from pinn_elastodynamics_amd.navier_cauchy_3d import LOSS_LAYOUT_3D, NavierCauchy3D, halfspace_case
from pinn_elastodynamics_amd.plate_hole import PINN
from tests import _refine_cases as RC
from tests._oracle_engine import OracleEngine
from tests.test_plate_host import LB, LD, LN, LP, UB, nets, plate_sets


class RefineEngine(OracleEngine):
    """OracleEngine with HipEngine's plate_residual_score / nc3d_residual_score / select_k: float64 oracle residuals on the streams the stand-in
    itself returns, rounded to fp32; the numpy selection reference"""

    def for_layers(self, layers):
        return RefineEngine(layers)

    def plate_residual_score(self, params, x, y, t, lb, ub, normalize, frozen, term_weights, E=20.0, mu=0.25, rho=1.0, out=None, packed=False):
        self.calls.append(("score", x.numel(), tuple(float(v) for v in term_weights), bool(packed)))
        fr = self._np(frozen)
        assert fr.shape == (2, 5, 5, x.numel())
        N = pl.net_streams(self._np(params), self.layers, self._np(x), self._np(y), self._np(t))
        f = pl.plate_residuals(pl.composite(N, fr[0], fr[1]), E, mu, rho)
        return torch.from_numpy(((f ** 2) @ np.asarray(term_weights, dtype=np.float64)).astype(np.float32))

    def nc3d_residual_score(self, params, x, y, z, t, lb, ub, normalize, term_weights, E=2.5, mu=0.25, rho=1.0, out=None, packed=False):
        self.calls.append(("score", x.numel(), tuple(float(v) for v in term_weights), bool(packed)))
        o = n3.nc3d_fields(self._np(params), self.layers, self._np(x), self._np(y), self._np(z), self._np(t), lb, ub, normalize)
        f = n3.nc3d_residuals(o["Y"], o["dY"], E, mu, rho)
        return torch.from_numpy(((f ** 2) @ np.asarray(term_weights, dtype=np.float64)).astype(np.float32))

    def select_k(self, score, k, largest=True):
        self.calls.append(("select", score.numel(), int(k), bool(largest)))
        return torch.from_numpy(RC.select_reference(score.numpy(), int(k), largest))


def fake_ranks(monkeypatch, rank, world):
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda group=None: rank)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: world)


# ---- plate ---------------------------------------------------------------------------------------------------------------------------------------
def plate_model(seed=2, n=120):
    _, rng = nets(seed)
    sets = plate_sets(rng, n)
    eng = {"uv": RefineEngine(LN), "dist": RefineEngine(LD), "part": RefineEngine(LP)}
    return PINN(*sets, LN, LD, LP, LB, UB, engines=eng, verbose=False, seed=seed), sets


def plate_candidates(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) * 0.5, rng.random(n) * 0.5, rng.random(n) * 10], 1)


def test_plate_refine_bookkeeping_and_frozen_columns():
    m, sets = plate_model()
    keep = sets[0].copy()
    cand = plate_candidates(50, 6)
    s_rows = m.residual_score(m.x_c, m.y_c, m.t_c)
    assert s_rows.shape == (120, 1) and m.eng["uv"].calls[-1][2] == (10.0,) * 5
    s_cand = m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1)
    rows, cands = RC.refine_rule(s_rows.reshape(-1), s_cand, 30)
    frozen0 = m._frozen_collo.clone()
    fc = torch.stack([m.eng[k].net_streams(m.theta[k], *[torch.from_numpy(cand[:, j].astype(np.float32)) for j in range(3)], LB, UB, False)
                      for k in ("dist", "part")])
    for e in m.eng.values():
        e.calls.clear()
    out = m.refine_collocation(cand, 30)
    calls = m.eng["uv"].calls
    assert [c[0] for c in calls] == ["score", "score", "select", "select"] and calls[1][3] is True        # the second score reuses the packed weights
    assert calls[0][1] == 120 and calls[1][1] == 50 and calls[2][1:] == (50, 30, True) and calls[3][1:] == (120, 30, False)
    assert set(out) == {"replaced", "rows", "candidate_indices", "score_replaced_max", "score_inserted_min"}
    assert out["replaced"] == rows.size > 0 and np.array_equal(out["rows"], rows) and np.array_equal(out["candidate_indices"], cands)
    assert out["score_replaced_max"] == float(s_rows.reshape(-1)[rows].max()) and out["score_inserted_min"] == float(s_cand[cands].min())
    want = keep.copy()
    want[rows] = cand[cands]
    assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1), want) and np.array_equal(sets[0], keep)     # the caller's array is not written
    assert np.array_equal(np.stack([a.numpy() for a in m._collo], axis=1), want.astype(np.float32)) and m.n_collo == 120
    # the frozen D / P streams followed the rows: replaced columns are the candidates', the others kept their bits, and a fresh evaluation agrees
    untouched = np.ones(120, dtype=bool)
    untouched[rows] = False
    assert torch.equal(m._frozen_collo[..., untouched], frozen0[..., untouched])
    assert torch.equal(m._frozen_collo[..., rows], fc[..., cands]) and m._frozen_collo.shape == (2, 5, 5, 120) and m._frozen_collo.is_contiguous()
    held = m._frozen_collo.clone()
    m.refresh_frozen()
    assert torch.equal(held, m._frozen_collo)
    # own weights, K capped by the candidates; nothing to do; argument checks
    out = m.refine_collocation(cand[:5], 30, weights=[1, 0, 0, 0, 2])
    assert calls[-1][1:] == (120, 5, False) and calls[-3][2] == (1.0, 0.0, 0.0, 0.0, 2.0) and out["replaced"] <= 5
    assert m.refine_collocation(cand, 0)["replaced"] == 0 and m.refine_collocation(np.zeros((0, 3)), 5)["score_replaced_max"] is None
    with pytest.raises(ValueError):
        m.refine_collocation(np.zeros((4, 4)), 2)
    with pytest.raises(ValueError):
        m.refine_collocation(cand, 2, weights=[1.0] * 7)
    with pytest.raises(ValueError):
        m.residual_score(m.x_c, m.y_c, m.t_c, weights=[1.0] * 4)
    assert np.isfinite(m.getloss()["loss"])


def test_plate_refine_touches_only_this_ranks_shard(monkeypatch):
    cand = plate_candidates(40, 8)
    for r in (0, 1):
        fake_ranks(monkeypatch, r, 2)
        m, sets = plate_model(n=101)
        lo, hi = m._shard(0, 101)
        assert m._collo[0].numel() == hi - lo and m._frozen_collo.shape[-1] == hi - lo
        s_rows = m.residual_score(m.x_c[lo:hi], m.y_c[lo:hi], m.t_c[lo:hi]).reshape(-1)
        s_cand = m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1)
        rows, cands = RC.refine_rule(s_rows, s_cand, 100)             # K = min(100, 40, rows of the shard)
        out = m.refine_collocation(cand, 100)
        assert m.eng["uv"].calls[-1][1:] == (hi - lo, 40, False)
        assert np.array_equal(out["rows"], rows + lo) and out["rows"].min() >= lo and out["rows"].max() < hi
        want = sets[0].copy()
        want[rows + lo] = cand[cands]
        assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1), want)
        assert np.array_equal(np.stack([a.numpy() for a in m._collo], axis=1), want[lo:hi].astype(np.float32))
        held = m._frozen_collo.clone()
        m.refresh_frozen()
        assert torch.equal(held, m._frozen_collo)


# ---- 3-D -------------------------------------------------------------------------------------------------------------------------------------------
def nc3d_model(n=301, **kw):
    c = halfspace_case(n_collo=n, n_ic=40, n_top=40, n_src=(6, 5), seed=4, width=16, depth=2)
    m = NavierCauchy3D(c["Collo"], c["SRC"], c["IC"], c["TOP"], c["uv_layers"], c["lb"], c["ub"], engine=RefineEngine(c["uv_layers"]), verbose=False,
                       seed=9, **kw)
    return c, m


def nc3d_candidates(c, n, seed):
    return n3.halfspace_points(n, c["lb"], c["ub"], np.random.default_rng(seed))


def test_nc3d_refine_bookkeeping_single_process():
    c, m = nc3d_model()
    keep = c["Collo"].copy()
    cand = nc3d_candidates(c, 60, 6)
    cols = lambda A: [A[:, k:k + 1] for k in range(4)]
    s_rows = m.residual_score(m.x_c, m.y_c, m.z_c, m.t_c)
    lay = LOSS_LAYOUT_3D
    assert s_rows.shape == (301, 1) and m.engine.calls[-1][2] == tuple([lay["f_uv"]] * 6 + [lay["f_s"]] * 6)
    s_cand = m.residual_score(*cols(cand)).reshape(-1)
    rows, cands = RC.refine_rule(s_rows.reshape(-1), s_cand, 40)
    m._rows(0, 150)
    m.engine.calls.clear()
    out = m.refine_collocation(cand, 40)
    calls = m.engine.calls
    assert [k[0] for k in calls] == ["score", "score", "select", "select"] and calls[1][3] is True
    assert calls[2][1:] == (60, 40, True) and calls[3][1:] == (301, 40, False)
    assert out["replaced"] == rows.size > 0 and np.array_equal(out["rows"], rows) and np.array_equal(out["candidate_indices"], cands)
    want = keep.copy()
    want[rows] = cand[cands]
    assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.z_c, m.t_c], axis=1), want) and np.array_equal(c["Collo"], keep)
    w32 = want.astype(np.float32)
    assert np.array_equal(np.stack(m._collo_host, axis=1), w32) and np.array_equal(np.stack([a.numpy() for a in m._rows(0, 301)], axis=1), w32)
    assert m._n_collo == 301
    out = m.refine_collocation(cand[:5], 40, weights=[1] + [0] * 11)
    assert calls[-1][1:] == (301, 5, False) and calls[-3][2] == (1.0,) + (0.0,) * 11 and out["replaced"] <= 5
    assert m.refine_collocation(cand, 0)["replaced"] == 0 and m.refine_collocation(np.zeros((0, 4)), 5)["score_replaced_max"] is None
    with pytest.raises(ValueError):
        m.refine_collocation(np.zeros((4, 3)), 2)
    with pytest.raises(ValueError):
        m.refine_collocation(cand, 2, weights=[1.0] * 7)
    assert np.isfinite(m.getloss()[0]) and np.isfinite(m.train(1, 1e-3, 2)[4]).all()


def test_nc3d_refine_touches_only_this_ranks_shard(monkeypatch):
    for r in (0, 1):
        fake_ranks(monkeypatch, r, 2)
        c, m = nc3d_model(n=201)
        cand = nc3d_candidates(c, 40, 8)
        lo, hi = m._shard(0, 201)
        cols = lambda A: [A[:, k:k + 1] for k in range(4)]
        s_rows = m.residual_score(*cols(c["Collo"][lo:hi])).reshape(-1)
        s_cand = m.residual_score(*cols(cand)).reshape(-1)
        rows, cands = RC.refine_rule(s_rows, s_cand, 150)
        out = m.refine_collocation(cand, 150)
        assert m.engine.calls[-1][1:] == (hi - lo, 40, False)
        assert np.array_equal(out["rows"], rows + lo) and out["rows"].min() >= lo and out["rows"].max() < hi
        want = c["Collo"].astype(np.float32)
        want[rows + lo] = cand[cands].astype(np.float32)
        assert np.array_equal(np.stack(m._collo_host, axis=1), want)
        assert np.array_equal(np.stack([a.numpy() for a in m._rows(0, 201)], axis=1), want[lo:hi])         # re-uploaded from the host copies
