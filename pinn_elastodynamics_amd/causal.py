"""Causal collocation sampling for the wave family (elastic_wave.DeepHPM, DeepHPMConfined): WHEN in time the collocation points sit, as
refine.py decides where in space.  A tanh net can drive the residual to zero at late times by fitting the trivial field there before the wave
has arrived; Wang, Sankaran and Perdikaris ("Respecting causality is all you need") weight the residual of a time slice by
w = exp(-eps * accumulated residual of all earlier slices).  A loss with 1/N weights over points DRAWN with density ~ w(t) estimates that
weighted loss, so the rows move and the step stays: the set's size, the 1/N weights, the block boundaries, the shards and every loss kernel
are what they were.

  profile   ``candidates`` probe points uniform in (lb, ub) on the stream  0x80000000 | round  -- the SAME on every rank; refinement's streams
            round * world + rank stay below bit 31 --, their residual score, -inf inside the excluded discs (refine_keys, mask mode), the
            per-time-bin sums and counts (binned_sums), and from them the weights and the CDF of max(w, floor) (causal_cdf).  Every rank holds the
            same parameters, so every rank gets the same table bit for bit with no collective, the way validate works.
  redraw    this rank's rows are drawn again from the table: N_shard + slack points on the rank's ordinary stream round * world + rank
            (sample_box(t_cdf=...)), mask keys of a constant score 1 against the excluded discs, select_k(largest) for N_shard -- its tie rule,
            lowest index first, makes that the first N_shard valid points.  A selected entry whose key is -inf is dropped; where fewer than
            N_shard are valid the remaining rows keep their old points.  No loop, no fallback draw.
  scale     ``ref="first"``: eps is divided by the mean score over all probe points of this model's FIRST profile, so it is dimensionless; a
            float uses that scale instead.
"""
from __future__ import annotations

import numpy as np
import torch

from .capi import MAX_TIME_BINS
from .refine import overwrite_rows

PROBE_STREAM = 0x80000000          # bit 31: the probe points' streams, apart from every round * world + rank


def check_discs(exclude):
    ex = [tuple(float(v) for v in b) for b in exclude]
    if any(len(b) != 3 for b in ex):
        raise ValueError("exclude: (xc, yc, r)")
    return ex


def profile_device(model, bins, candidates, w, exclude=(), seed=None):
    """the four device calls of a profile: the device float64 tensor [2, bins] of the per-bin score sums and counts.  No download."""
    bins, n = int(bins), int(candidates)
    if not 1 <= bins <= MAX_TIME_BINS:
        raise ValueError(f"bins: 1 .. {MAX_TIME_BINS}")
    if n < 1:
        raise ValueError("candidates: at least one probe point")
    eng, seed = model.engine, 0 if seed is None else int(seed)
    stream = PROBE_STREAM | getattr(model, "_refine_round", 0)
    lo, hi = [float(v) for v in model.lb], [float(v) for v in model.ub]
    cols = eng.sample_box(n, lo, hi, seed, stream)
    # (not packed=True: behind a training step the workspace holds the packed form of the weights BEFORE the update)
    score = model._score_device(cols, w)
    keys = eng.refine_keys(score, cols, check_discs(exclude), "mask", 1.0, 1.0, seed, stream)
    return eng.binned_sums(keys, cols[-1], lo[-1], hi[-1], bins)


def profile_host(binned):
    """host [2, bins] sums and counts -> (per-bin mean, 0 where a bin is empty; counts)"""
    s = np.asarray(binned, dtype=np.float64)
    return np.divide(s[0], s[1], out=np.zeros_like(s[0]), where=s[1] > 0), s[1].copy()


def reference_scale(binned):
    """the mean score over all the probe points of a host [2, bins] profile; 1 where that is not a positive finite number"""
    s = np.asarray(binned, dtype=np.float64)
    m = s[0].sum() / s[1].sum() if s[1].sum() > 0 else 0.0
    return float(m) if np.isfinite(m) and m > 0 else 1.0


def residual_profile(model, bins, candidates, weights=None, *, exclude=(), seed=None):
    """DeepHPM.residual_profile"""
    return profile_host(profile_device(model, bins, candidates, model._score_weights(weights), exclude, seed).cpu().numpy())


class CausalArgs:
    """the entries of resample_collocation's / train's ``causal`` dict, checked"""
    KEYS = ("bins", "eps", "candidates", "floor", "exclude", "seed", "ref", "weights", "slack")

    def __init__(self, model, causal):
        kw = dict(causal)
        try:
            self.bins, self.eps, self.candidates = int(kw.pop("bins")), float(kw.pop("eps")), kw.pop("candidates")
        except KeyError as e:
            raise ValueError(f"causal: missing {e.args[0]!r} (need bins, eps, candidates)") from None
        self.floor, self.exclude, self.seed = float(kw.pop("floor", 0.0)), check_discs(kw.pop("exclude", ())), kw.pop("seed", None)
        self.ref, self.slack = kw.pop("ref", "first"), kw.pop("slack", None)
        self.w = model._score_weights(kw.pop("weights", None))
        if kw:
            raise ValueError(f"causal: unknown entries {sorted(kw)}")
        if not 1 <= self.bins <= MAX_TIME_BINS:
            raise ValueError(f"causal: bins in 1 .. {MAX_TIME_BINS}")
        if not (np.isfinite(self.eps) and self.eps >= 0 and np.isfinite(self.floor) and self.floor >= 0):
            raise ValueError("causal: eps and floor finite and not negative")
        if not isinstance(self.candidates, (int, np.integer)) or isinstance(self.candidates, bool) or self.candidates < 1:
            raise ValueError("causal: candidates an int >= 1 (probe points drawn on the device)")
        if self.ref != "first" and not (isinstance(self.ref, (int, float)) and np.isfinite(self.ref) and self.ref > 0):
            raise ValueError("causal: ref is 'first' or a positive score scale")
        if self.slack is not None and int(self.slack) < 0:
            raise ValueError("causal: slack >= 0")

    def scale(self, model):
        """the score scale eps is divided by, or None while ref='first' has not been fetched"""
        return getattr(model, "_causal_ref", None) if self.ref == "first" else float(self.ref)


def redraw(model, a, binned, scale, names):
    """The table from the device profile ``binned`` and this rank's rows drawn again from it (module docstring).  Synchronises with the host:
    the boolean index below waits for the count of valid points, and the redrawn rows' indices and points are downloaded -- the
    bookkeeping of refine.overwrite_rows.  Nothing of the profile or the table comes down.  Returns (redrawn, w, cdf), the last two on the
    device."""
    eng = model.engine
    w, cdf = eng.causal_cdf(binned, a.eps / scale, a.floor)
    model._causal_cdf = cdf
    rnd = getattr(model, "_refine_round", 0)
    model._refine_round = rnd + 1
    s0, e0 = model._shard(0, model._n_collo)
    n_shard = e0 - s0
    if n_shard <= 0:
        return 0, w, cdf
    seed, stream = 0 if a.seed is None else int(a.seed), rnd * model.world + model.rank
    n_draw = n_shard + (n_shard // 8 + 64 if a.slack is None else int(a.slack))
    cols = eng.sample_box(n_draw, [float(v) for v in model.lb], [float(v) for v in model.ub], seed, stream, t_cdf=cdf)
    keys = eng.refine_keys(torch.ones(n_draw, dtype=torch.float32, device=cols[0].device), cols, a.exclude, "mask", 1.0, 1.0, seed, stream)
    sel = eng.select_k(keys, n_shard, largest=True).long()
    ci = sel[keys[sel] > float("-inf")]
    ri = torch.arange(ci.numel(), dtype=torch.int64, device=ci.device)
    moved = overwrite_rows(model, names, s0, ri, cols, ci,
                           lambda cand, idx, c_host: torch.stack([c[idx] for c in cand], dim=1).cpu().numpy().astype(np.float64))
    return (0 if moved is None else len(moved[0])), w, cdf


def resample_collocation(model, causal, names):
    """DeepHPM.resample_collocation"""
    a = CausalArgs(model, causal)
    binned = profile_device(model, a.bins, a.candidates, a.w, a.exclude, a.seed)
    host = binned.cpu().numpy()
    if a.scale(model) is None:
        model._causal_ref = reference_scale(host)          # once per model
    n_shard = model._shard(0, model._n_collo)
    n_shard = n_shard[1] - n_shard[0]
    m, w, cdf = redraw(model, a, binned, a.scale(model), names)
    profile, counts = profile_host(host)
    return {"redrawn": m, "kept": n_shard - m, "w": w.cpu().numpy(), "cdf": cdf.cpu().numpy(), "profile": profile, "counts": counts}


class CausalSchedule:
    """train(..., causal=dict(every=E, bins, eps, candidates, floor=0.0, exclude=(), seed=None, ref="first")): the profile, the table and the
    redraw behind every E-th step of the call, in front of refinement's hook.  ``after_step(j)`` with j = 1, 2, ... counted over the whole
    train call.  Every trigger redraws, the first one of a fresh model included: while ``ref="first"`` has no scale yet, that trigger
    fetches its own profile (2 * bins doubles: one download, once per model) and takes the scale from it.  Apart from that the profile, the
    weights and the table stay on the device.  The redraw itself synchronises with the host once per trigger, as refinement does: how many
    of the drawn points are valid, and the redrawn rows for the host copies of the set (redraw)."""

    def __init__(self, model, causal, names):
        kw = dict(causal)
        try:
            self.every = int(kw.pop("every"))
        except KeyError:
            raise ValueError("causal: missing 'every'") from None
        if self.every < 1:
            raise ValueError("causal: every >= 1")
        self.model, self.args, self.names = model, CausalArgs(model, kw), names
        self.redrawn = []

    def after_step(self, step):
        if step % self.every != 0:
            return
        m, a = self.model, self.args
        binned = profile_device(m, a.bins, a.candidates, a.w, a.exclude, a.seed)
        if a.scale(m) is None:
            m._causal_ref = reference_scale(binned.cpu().numpy())          # once per model
        self.redrawn.append(redraw(m, a, binned, a.scale(m), self.names)[0])


def schedule(model, causal, names):
    """the CausalSchedule of train(causal=...), or None for causal=None"""
    return None if causal is None else CausalSchedule(model, causal, names)
