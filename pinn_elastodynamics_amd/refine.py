"""Residual-adaptive refinement of a collocation set: what the model classes share (elastic_wave.DeepHPM, navier_cauchy_3d.NavierCauchy3D,
plate_hole.PINN).  The rule: score this rank's rows and the candidates on the device, take the K = min(n_replace, candidates, rows)
highest-scoring candidates and the K lowest-scoring rows (engine.select_k), pair them -- highest candidate against lowest row -- and overwrite
a row ONLY where its candidate scores strictly higher.  The set keeps its size, so the 1/N weights, the block boundaries of train(batch_num),
the workspace and the data-parallel shards stay what they were.  No collective: every rank refines its own rows with the candidates it is given.
Candidates may also be DRAWN ON THE DEVICE (an int instead of an array: engine.sample_box, stream = round * world + rank, so ranks and rounds get
distinct, reproducible points), regions may be excluded, and the K candidates may be drawn with probability ~ score^power / mean + c instead of
taken greedily (engine.refine_keys turns the scores into keys, select_k then runs on the keys).  The rule for the rows stays: a candidate goes in
only where its SCORE is strictly larger than the row's, and an excluded candidate (key -inf) never does.
"""
from __future__ import annotations

import numpy as np
import torch

from .optim import device_column


def pair_replacements(cand_idx, cand_score, row_idx, row_score):
    """The pairing rule of refine_collocation on the K selected candidates and the K selected rows (torch tensors on any device; the index
    tensors ascending, as select_k returns them): candidates by score descending, rows by score ascending -- ties by index ascending in
    both --, pair j = (row j, candidate j), kept ONLY where the candidate's score is strictly larger than the row's.  A NaN score never
    satisfies that.  Returns (rows, candidates, row scores, candidate scores) of the kept pairs, in pairing order."""
    oc = torch.sort(cand_score, descending=True, stable=True).indices
    orr = torch.sort(row_score, descending=False, stable=True).indices
    ci, cs, ri, rs = cand_idx[oc], cand_score[oc], row_idx[orr], row_score[orr]
    keep = cs > rs
    return ri[keep], ci[keep], rs[keep], cs[keep]


def score_weights(weights, default, what):
    """``default`` unless the caller gives one weight per residual (``what`` names them in the error)"""
    if weights is None:
        return list(default)
    w = [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
    if len(w) != len(default):
        raise ValueError(f"weights: one per residual of net_f_sig {what}")
    return w


def candidate_array(candidates, ncols, names):
    C = np.asarray(candidates, dtype=np.float64)
    if C.ndim != 2 or C.shape[1] != ncols:
        raise ValueError(f"candidates must be [Nc, {ncols}] = {names}")
    return C


def device_columns(C, device):
    return tuple(device_column(C[:, k], device) for k in range(C.shape[1]))


def empty_result():
    return {"replaced": 0, "rows": np.zeros(0, dtype=np.int64), "candidate_indices": np.zeros(0, dtype=np.int64),
            "score_replaced_max": None, "score_inserted_min": None}


def pair_by_key(cand_idx, cand_key, cand_score, row_idx, row_score):
    """pair_replacements where the candidates were selected by a KEY (engine.refine_keys) that is not their score: candidates by key descending,
    rows by score ascending, pair j kept only where the candidate's SCORE is strictly larger than the row's and its key is not -inf (an excluded
    candidate, selected because fewer than K were valid, is never inserted)."""
    oc = torch.sort(cand_key, descending=True, stable=True).indices
    orr = torch.sort(row_score, descending=False, stable=True).indices
    ci, ck, cs, ri, rs = cand_idx[oc], cand_key[oc], cand_score[oc], row_idx[orr], row_score[orr]
    keep = (cs > rs) & (ck > float("-inf"))
    return ri[keep], ci[keep], rs[keep], cs[keep]


def select_pairs(engine, s_rows, s_cand, K, keys=None):
    """the two selections and the pairing on the device: (rows, candidates, row scores, candidate scores) of the pairs to replace; with
    ``keys`` the candidates are selected and ordered by them (pair_by_key)"""
    ci = engine.select_k(s_cand if keys is None else keys, K, largest=True).long()
    ri = engine.select_k(s_rows, K, largest=False).long()
    if keys is None:
        return pair_replacements(ci, s_cand[ci], ri, s_rows[ri])
    return pair_by_key(ci, keys[ci], s_cand[ci], ri, s_rows[ri])


class Candidates:
    """The candidates of one refine_collocation call.  ``candidates``: a float64 [Nc, ncols] array (converted and uploaded by ``columns``) or an
    int: that many points drawn on the device in ``box`` = (lo, hi) -- default the model's (lb, ub) -- by engine.sample_box(seed, stream), the
    stream by default  round * world + rank  with ``round`` the model's count of device-drawn refinements so far.  ``plain``: an array, greedy
    selection, nothing excluded -- the path that existed before keys did, which makes the engine calls it always made.  ``causal``: the drawn
    points' time column follows the model's current causal table (model._causal_cdf, causal.py) over the box's time range instead of the
    uniform law; without a table, or with an array, ValueError."""

    def __init__(self, model, candidates, ncols, names, select="top", power=1.0, c=1.0, seed=None, stream=None, box=None, exclude=(), causal=False):
        if select not in ("top", "sample"):
            raise ValueError("select must be 'top' or 'sample'")
        self.t_cdf = getattr(model, "_causal_cdf", None) if causal else None
        if causal and (self.t_cdf is None or not (isinstance(candidates, (int, np.integer)) and not isinstance(candidates, bool))):
            raise ValueError("causal=True needs an int number of candidates and a table: call resample_collocation(causal=...) or train(causal=...) first")
        self.select, self.power, self.c = select, float(power), float(c)
        self.exclude = [tuple(float(v) for v in b) for b in exclude]
        for b in self.exclude:
            if len(b) != 3 and not (len(b) == 4 and ncols == 4):
                raise ValueError("exclude: (xc, yc, r)" + (" or (xc, yc, zc, r)" if ncols == 4 else ""))
        self.seed = 0 if seed is None else int(seed)
        self.drawn = isinstance(candidates, (int, np.integer)) and not isinstance(candidates, bool)
        self.stream = 0 if stream is None else int(stream)
        if self.drawn:
            self.C, self.n = None, int(candidates)
            if self.n < 0:
                raise ValueError("candidates: a number of points to draw must not be negative")
            rnd = getattr(model, "_refine_round", 0)
            model._refine_round = rnd + 1
            if stream is None:
                self.stream = rnd * model.world + model.rank
            lo, hi = (model.lb, model.ub) if box is None else box
            self.lo, self.hi = ([float(v) for v in np.asarray(b, dtype=np.float64).reshape(-1)] for b in (lo, hi))
            if len(self.lo) != ncols or len(self.hi) != ncols:
                raise ValueError(f"box: (lo, hi) with {ncols} bounds each = {names}")
        else:
            self.C = candidate_array(candidates, ncols, names)
            self.n = self.C.shape[0]
        self.plain = not self.drawn and select == "top" and not self.exclude

    def columns(self, engine, device):
        """the candidates as device columns"""
        if self.drawn and self.t_cdf is not None:
            return engine.sample_box(self.n, self.lo, self.hi, self.seed, self.stream, t_cdf=self.t_cdf)
        if self.drawn:
            return engine.sample_box(self.n, self.lo, self.hi, self.seed, self.stream)
        return device_columns(self.C, device)

    def keys(self, engine, s_cand, cols):
        """what select_k runs on: None on the plain path (the scores themselves), else engine.refine_keys of the scores"""
        if self.plain:
            return None
        return engine.refine_keys(s_cand, cols, self.exclude, "sample" if self.select == "sample" else "mask", self.power, self.c, self.seed, self.stream)

    def inserted(self, cols, ci, c_host):
        """the inserted points as a host [m, ncols] float64 array (pairing order)"""
        if self.C is not None:
            return self.C[c_host]
        return torch.stack([a[ci] for a in cols], dim=1).cpu().numpy().astype(np.float64)


class RefineSchedule:
    """train(..., refine=dict(every=E, candidates=Nc, n_replace=K, **keywords of refine_collocation)): refine_collocation behind every E-th
    step of the call.  ``after_step(j)`` with j = 1, 2, ... counted over the whole train call."""

    def __init__(self, model, refine):
        kw = dict(refine)
        try:
            self.every, cand, n_replace = int(kw.pop("every")), kw.pop("candidates"), int(kw.pop("n_replace"))
        except KeyError as e:
            raise ValueError(f"refine: missing {e.args[0]!r} (need every, candidates, n_replace)") from None
        if self.every < 1 or not isinstance(cand, (int, np.integer)) or isinstance(cand, bool):
            raise ValueError("refine: every >= 1 and candidates an int (points drawn on the device each time)")
        self.model, self.args, self.kw, self.results = model, (int(cand), n_replace), kw, []

    def after_step(self, step):
        if step % self.every == 0:
            self.results.append(self.model.refine_collocation(*self.args, **self.kw))


def schedule(model, refine):
    """the RefineSchedule of train(refine=...), or None for refine=None"""
    return None if refine is None else RefineSchedule(model, refine)


def update_host_columns(model, names, r_host, c_host, C):
    """the [N,1] host columns ``names`` of the model follow the replacement -- on copies: they may be views of the caller's array"""
    if not getattr(model, "_collo_cols_owned", False):
        for nm in names:
            setattr(model, nm, getattr(model, nm).copy())
        model._collo_cols_owned = True
    for k, nm in enumerate(names):
        getattr(model, nm)[r_host, 0] = C[c_host, k]


def overwrite_rows(model, names, s0, ri, cand, ci, inserted):
    """Rows ``s0 + ri`` of the sharded set (``s0``: the first row of this rank's shard; ``ri``, ``ci`` device index tensors of one length) take
    the points ``cand[k][ci]`` of the device columns ``cand``: the device set (_collo_full), the host columns ``names`` and _collo_host
    follow, the shard cache is dropped.  ``inserted(cand, ci, c_host)`` gives the points as a host [m, len(names)] float64 array.  One
    download (the indices, and the points where only the device has them).  Returns (rows, candidate indices, points) on the host, or None
    where nothing moves.  Shared by refinement (below) and the causal redraw (causal.py)."""
    m = int(ri.numel())
    model._collo_cache = {}
    if m == 0:
        return None
    if model._collo_full is not None:
        for k in range(len(names)):
            model._collo_full[k][s0 + ri] = cand[k][ci]
    r_host, c_host = ri.cpu().numpy() + s0, ci.cpu().numpy()
    pts = inserted(cand, ci, c_host)
    update_host_columns(model, names, r_host, np.arange(m), pts)
    for k in range(len(names)):
        model._collo_host[k][r_host] = pts[:, k].astype(np.float32)
    return r_host, c_host, pts


def refine_sharded_set(model, C, n_replace, w, names):
    """refine_collocation of the classes that keep the set as host columns plus device shards (_collo_host / _collo_full / _collo_cache, _rows,
    _shard, _n_collo) and score through ``model._score_device(columns, weights, packed=...)``.  ``C``: a Candidates, or candidates
    [Nc, len(names)] float64."""
    if not isinstance(C, Candidates):
        C = Candidates(model, C, len(names), names)
    s0, e0 = model._shard(0, model._n_collo)
    K = min(int(n_replace), C.n, e0 - s0)
    out = empty_result()
    if not C.plain:
        out["candidates"] = np.zeros((0, len(names)))
    if K <= 0:
        return out
    rows = model._rows(0, model._n_collo)
    cand = C.columns(model.engine, model.device)
    s_rows = model._score_device(rows, w)
    s_cand = model._score_device(cand, w, packed=True)
    ri, ci, rs, cs = select_pairs(model.engine, s_rows, s_cand, K, C.keys(model.engine, s_cand, cand))
    moved = overwrite_rows(model, names, s0, ri, cand, ci, C.inserted)
    if moved is None:
        return out
    r_host, c_host, pts = moved
    out.update(replaced=len(r_host), rows=r_host, candidate_indices=c_host, score_replaced_max=float(rs.max()), score_inserted_min=float(cs.min()))
    if not C.plain:
        out["candidates"] = pts
    return out
