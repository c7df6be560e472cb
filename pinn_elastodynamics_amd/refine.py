"""Residual-adaptive refinement of a collocation set: what the model classes share (elastic_wave.DeepHPM, navier_cauchy_3d.NavierCauchy3D,
plate_hole.PINN).  The rule: score this rank's rows and the candidates on the device, take the K = min(n_replace, candidates, rows)
highest-scoring candidates and the K lowest-scoring rows (engine.select_k), pair them -- highest candidate against lowest row -- and overwrite
a row ONLY where its candidate scores strictly higher.  The set keeps its size, so the 1/N weights, the block boundaries of train(batch_num),
the workspace and the data-parallel shards stay what they were.  No collective: every rank refines its own rows with the candidates it is given.
"""
from __future__ import annotations

import numpy as np
import torch


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
    return tuple(torch.from_numpy(np.ascontiguousarray(C[:, k], dtype=np.float32)).to(device) for k in range(C.shape[1]))


def empty_result():
    return {"replaced": 0, "rows": np.zeros(0, dtype=np.int64), "candidate_indices": np.zeros(0, dtype=np.int64),
            "score_replaced_max": None, "score_inserted_min": None}


def select_pairs(engine, s_rows, s_cand, K):
    """the two selections and the pairing on the device: (rows, candidates, row scores, candidate scores) of the pairs to replace"""
    ci = engine.select_k(s_cand, K, largest=True).long()
    ri = engine.select_k(s_rows, K, largest=False).long()
    return pair_replacements(ci, s_cand[ci], ri, s_rows[ri])


def update_host_columns(model, names, r_host, c_host, C):
    """the [N,1] host columns ``names`` of the model follow the replacement -- on copies: they may be views of the caller's array"""
    if not getattr(model, "_collo_cols_owned", False):
        for nm in names:
            setattr(model, nm, getattr(model, nm).copy())
        model._collo_cols_owned = True
    for k, nm in enumerate(names):
        getattr(model, nm)[r_host, 0] = C[c_host, k]


def refine_sharded_set(model, C, n_replace, w, names):
    """refine_collocation of the classes that keep the set as host columns plus device shards (_collo_host / _collo_full / _collo_cache, _rows,
    _shard, _n_collo) and score through ``model._score_device(columns, weights, packed=...)``.  ``C``: candidates [Nc, len(names)] float64."""
    s0, e0 = model._shard(0, model._n_collo)
    K = min(int(n_replace), C.shape[0], e0 - s0)
    out = empty_result()
    if K <= 0:
        return out
    rows = model._rows(0, model._n_collo)
    cand = device_columns(C, model.device)
    s_rows = model._score_device(rows, w)
    s_cand = model._score_device(cand, w, packed=True)
    ri, ci, rs, cs = select_pairs(model.engine, s_rows, s_cand, K)
    m = int(ri.numel())
    model._collo_cache = {}
    if m == 0:
        return out
    if model._collo_full is not None:
        for k in range(len(names)):
            model._collo_full[k][s0 + ri] = cand[k][ci]
    r_host, c_host = ri.cpu().numpy() + s0, ci.cpu().numpy()
    update_host_columns(model, names, r_host, c_host, C)
    for k in range(len(names)):
        model._collo_host[k][r_host] = C[c_host, k].astype(np.float32)
    out.update(replaced=m, rows=r_host, candidate_indices=c_host, score_replaced_max=float(rs.max()), score_inserted_min=float(cs.min()))
    return out
