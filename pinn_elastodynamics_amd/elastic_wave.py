"""Host-side mirror of the reference's model class for the three elastic-wave cases.

Same names, argument order and column-tensor convention as ``class DeepHPM`` in
  INF  = ElasticWaveInfinite/ElasticWave.py      (float32, inputs normalised, INF:191)
  SEMI = ElasticWaveSemiInfinite/ElasticWave.py  (raw inputs, loss layout SEMI:127)
  CONF = ElasticWaveConfined/ElasticWave.py      (raw inputs, FIXED edges, CONF:156)
but nothing of TF1's runtime: weights live in one flat fp32 device vector, point sets are device
resident (no per-step feed, cf. INF:297-305), the loss + gradient of every term comes from the
HIP kernels behind ``include/pinn_hip.h`` and Adam runs on the device.

Data-parallel training (one process per GPU, torch.distributed): every point set is sharded into
contiguous row ranges (the reference's own batching precedent, INF:292-297); each rank's kernels
weight their partial sums with the GLOBAL 1/N, one all-reduce(sum) of [flat gradient | loss sums]
follows, and the identical fused Adam step runs on every rank, so the weights stay bit-identical.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import causal as causal_sampling
from . import material
from .model_base import ShardedSetsModel
from .net_api import write_checkpoint
# (the optimizer and parameter helpers lived in this module before optim.py: tools and tests import them from here)
from .optim import (BFGS_BACKENDS, LbfgsResult, all_reduce_sum, check_backend, device_array, evaluate_with_finite_gradient, lbfgs_hip, lbfgs_on_device,  # noqa: F401
                    pack_params, relax_adjoint_shift, unpack_params, xavier_init)
from .refine import Candidates, candidate_array, pair_replacements, refine_sharded_set, schedule, score_weights  # noqa: F401
from .validate import PredictMixin, schedule as validate_schedule

# multipliers of (loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss_NB, loss_FIX) in the total loss
LOSS_LAYOUT = {
    "infinite": dict(f_uv=1.0, f_s=1.0, IC=1.0, SRC=1.0, NB=0.0, FIX=0.0),        # INF:119 (loss_NB excluded)
    "semi_infinite": dict(f_uv=5.0, f_s=5.0, IC=2.0, SRC=2.0, NB=2.0, FIX=0.0),   # SEMI:127
    "confined": dict(f_uv=5.0, f_s=5.0, IC=1.0, SRC=1.0, NB=0.0, FIX=1.0),        # CONF:156
}
# scipy L-BFGS-B options of tf.contrib.opt.ScipyOptimizerInterface (INF:122-129, SEMI:130-137, CONF:159-166)
_EPS = float(np.finfo(float).eps)
BFGS_OPTIONS = {
    "infinite": dict(maxiter=10000, maxfun=10000, maxcor=50, maxls=50, ftol=0.001 * _EPS),
    "semi_infinite": dict(maxiter=1000, maxfun=1000, maxcor=50, maxls=50, ftol=0.001 * _EPS),
    "confined": dict(maxiter=100000, maxfun=100000, maxcor=50, maxls=50, ftol=1.0 * _EPS),
}
_SLOTS = ("collo", "IC", "SRC", "NB", "FIX")   # 8 floats each in the loss-sum buffer


class DeepHPM(ShardedSetsModel, PredictMixin, material.MaterialMixin):
    """Drop-in for the reference's model class on the wave cases (INF:21-376)."""
    N_IN, COLLO_NAMES = 3, ("x_c", "y_c", "t_c")
    COLLO_TERMS, SUMS_STRIDE, SLOTS = (4, 3), 8, _SLOTS

    def __init__(self, Collo, SRC, IC, UP, uv_layers, lb, ub, ExistModel=0, modelDir='', *, case="infinite",
                 FIX=None, precision="f16x3", engine=None, seed=1111, process_group=None, verbose=True,
                 E=2.5, mu=0.25, rho=1.0, always_reduce=False, shard_as=None, collective="rccl", step_call=True, p2p_timeout_s=None,
                 TRAC=None, trac_weight=None):
        """``TRAC``: a traction boundary set [n, 5] = (x, y, t, nx, ny) -- traction-free: a cavity, an inclined or curved free surface -- or
        [n, 7] = (x, y, t, nx, ny, tx, ty) with a prescribed traction per point (pointsets.circle_traction_set / traction_set).  Its term
        loss_TRAC = <r_x^2> + <r_y^2>, r = sigma n - t of net_surf_var (INF:267-276), enters the total with ``trac_weight`` (default: what the
        case's layout puts on SRC).  The normals are used as given.  Without it the model is exactly the one without the keyword."""
        self.count = 0                      # callback counter (INF:26)
        self._step_call = bool(step_call)   # False: the step as separate library calls (collocation, side sets, Adam) -- the same bits; for A / B timing
        self._shift_state = {}              # adjoint-shift bookkeeping of evaluate_with_finite_gradient
        self.loss_rec = []                  # SEMI:39
        self.trac_rec = []                  # loss_TRAC per step of train() (models with a traction set)
        self.case = case
        self.layout = LOSS_LAYOUT[case]
        self.normalize = case == "infinite"            # INF:191 vs SEMI:198 / CONF:235
        self.lb = np.asarray(lb, dtype=np.float64).reshape(-1)
        self.ub = np.asarray(ub, dtype=np.float64).reshape(-1)
        self.E, self.mu, self.rho = E, mu, rho         # INF:33-35
        self.uv_layers = [int(v) for v in uv_layers]
        self.verbose = verbose

        self._init_topology(process_group, always_reduce, shard_as)
        # engine (GPU kernels); tests may inject a stand-in with the same methods
        self._set_engine(self._default_engine(self.uv_layers, precision, np.asarray(Collo).shape[0]) if engine is None else engine, "wave")
        self._init_net(seed, ExistModel, modelDir)

        # ---- point sets, column split like INF:40-59, stored SoA on the device
        self._init_collocation(Collo)
        self._add_side("IC", IC, (0, 1, 2, 3))                     # u,v,ut,vt = 0 at t=0          INF:111-114
        self._add_side("SRC", SRC, (0, 1), (3, 4))                 # u,v = source displacement     INF:115-116
        self._add_side("NB", UP, (5, 6))                           # s22,s12 = 0 on the free edge  INF:117-118
        self._add_side("FIX", FIX, (0, 1))                         # u,v = 0 on the fixed edges    CONF:145-146
        self.SRC, self.IC, self.UP, self.FIX = SRC, IC, UP, FIX
        self._add_traction(TRAC, trac_weight)                      # sigma n = t on a boundary with normals INF:267-276

        self._buf = torch.zeros(self.n_params + 8 * len(self.SLOTS), dtype=torch.float32, device=self.device)
        self._init_collective(collective, p2p_timeout_s)

    def _add_traction(self, TRAC, trac_weight):
        """Register the traction set: one more slot ("TRAC", sums r_x^2, r_y^2 in its columns 0, 1) behind the five every model has -- per
        instance, a model without the set keeps five --, this rank's rows and their [4, m] = nx, ny, tx, ty on the device, sharded as _add_side
        shards (the kernels weight with the global 1/n)."""
        self.TRAC = TRAC
        if TRAC is None or np.asarray(TRAC).shape[0] == 0:
            return
        A = np.asarray(TRAC, dtype=np.float64)
        if A.ndim != 2 or A.shape[1] not in (5, 7):
            raise ValueError("TRAC is [n, 5] = (x, y, t, nx, ny) or [n, 7] = (x, y, t, nx, ny, tx, ty)")
        self.SLOTS = _SLOTS + ("TRAC",)
        self.layout = dict(self.layout, TRAC=float(self.layout["SRC"] if trac_weight is None else trac_weight))
        n_glob = A.shape[0]
        s, e = self._shard(0, n_glob)
        A = A[s:e]
        aux = np.zeros((4, A.shape[0]), dtype=np.float32)
        aux[:A.shape[1] - 3] = A[:, 3:].T
        self._sides["TRAC"] = tuple(self._device_columns(A[:, k] for k in range(3))) + (device_array(aux, self.device), (0, 1), n_glob)

    def set_weights(self, weights, biases):
        self.theta.copy_(torch.from_numpy(pack_params(weights, biases)).to(self.device))

    # ------------------------------------------------------------------------------------------
    # graph pieces as callables on column arrays [N,1] (INF:188-276)
    # ------------------------------------------------------------------------------------------
    def _fields(self, x, y, t):
        xs = self._device_columns((x, y, t))
        return self.engine.fields(self.theta, xs[0], xs[1], xs[2], self.lb, self.ub, self.normalize)   # [4,7,N]

    # neural_net(X, weights, biases): net_api.NetApi, through _current_theta and this
    def _net_fields(self, eng, theta, X):
        xs = self._device_columns((X[:, k] for k in range(3)), eng.device)
        return eng.fields(theta, xs[0], xs[1], xs[2], self.lb, self.ub, self.normalize)[0]

    def net_uv(self, x, y, t):                       # INF:201-211
        return self._cols(self._fields(x, y, t)[0])

    def net_e(self, x, y, t):                        # INF:213-219
        F = self._fields(x, y, t)
        e11, e22, e12 = F[1, 0], F[2, 1], F[2, 0] + F[1, 1]
        return self._cols(torch.stack([e11, e22, e12]))

    def net_f_sig(self, x, y, t):                    # INF:221-265
        F = self._fields(x, y, t)
        return self._cols(self._residuals(F))

    def _residuals(self, F):
        E, mu, rho = self.E, self.mu, self.rho
        V, X, Y, T = F[0], F[1], F[2], F[3]
        e11, e22, e12 = X[0], Y[1], Y[0] + X[1]
        coef = E / ((1 + mu) * (1 - 2 * mu))                         # plane strain, INF:238
        sp11 = coef * (1 - mu) * e11 + coef * mu * e22
        sp22 = coef * mu * e11 + coef * (1 - mu) * e22
        sp12 = E / (2 * (1 + mu)) * e12
        f_u = X[4] + Y[6] - rho * T[2]
        f_v = Y[5] + X[6] - rho * T[3]
        return torch.stack([f_u, f_v, T[0] - V[2], T[1] - V[3], V[4] - sp11, V[5] - sp22, V[6] - sp12])

    # BASELINE.json's north_star calls these net_uvp / net_f; the reference's names are net_uv / net_f_sig
    net_uvp = net_uv
    net_f = net_f_sig

    def net_surf_var(self, x, y, t, nx, ny):         # INF:267-276
        u, v, ut, vt, s11, s22, s12 = self.net_uv(x, y, t)
        return s11 * nx + s12 * ny, s12 * nx + s22 * ny

    # ------------------------------------------------------------------------------------------
    # residual-adaptive refinement of the collocation set
    # ------------------------------------------------------------------------------------------
    def _score_weights(self, weights):
        """the coefficients the case's LOSS_LAYOUT puts on the seven collocation terms, unless the caller gives seven of its own"""
        return score_weights(weights, [self.layout["f_uv"]] * 4 + [self.layout["f_s"]] * 3, "(f_u, f_v, f_ut, f_vt, f_s11, f_s22, f_s12)")

    def _score_device(self, xs, w, packed=False):
        kw = {"packed": True} if packed else {}
        return self.engine.residual_score(self.theta, xs[0], xs[1], xs[2], self.lb, self.ub, self.normalize, w, self.E, self.mu, self.rho, True, **kw)

    def residual_score(self, x, y, t, weights=None):
        """sum_i weights[i] * f_i^2 of net_f_sig's seven residuals (INF:221-265) per point, numpy [N,1], formed on the device: the measure
        refine_collocation ranks by.  Default ``weights``: what the case's loss layout puts on the collocation terms."""
        xs = self._device_columns((x, y, t))
        return self._score_device(xs, self._score_weights(weights)).detach().cpu().numpy().reshape(-1, 1)

    def refine_collocation(self, candidates, n_replace, weights=None, *, select="top", power=1.0, c=1.0, seed=None, stream=None, box=None, exclude=(),
                           causal=False):
        """Residual-adaptive refinement that keeps the set's size: score this rank's rows of the collocation set and the ``candidates``
        [Nc,3] (x, y, t) on the device, take the K = min(n_replace, Nc, rows) highest-scoring candidates and the K lowest-scoring rows
        (engine.select_k), pair them (pair_replacements: highest candidate against lowest row) and overwrite row j with candidate j only
        where the candidate's score is strictly larger.  N, the 1/N weights, the block boundaries of train(batch_num), the workspace and the
        data-parallel shards stay what they were; the host copies (x_c, y_c, t_c) follow.
        Data parallel: no collective -- every rank refines ITS OWN rows with the candidates IT is given, so callers must pass rank-distinct
        candidates (the same candidates on every rank would be inserted once per rank).  The host copies of a rank then show its own
        replacements only, which is all that rank ever uploads.
        ``candidates`` may be an INT: that many points are drawn on the device in ``box`` = (lo, hi), default (lb, ub), by
        engine.sample_box(seed, stream) -- counter-based, so the points are a function of (seed, stream, index) alone; ``stream`` defaults to
        round * world + rank, ``round`` counting this model's device-drawn refinements: ranks and rounds get distinct, reproducible candidates
        with no coordination.  ``exclude``: discs (xc, yc, r) whose inside and boundary never enter the set (the source disc, a hole: single
        points there reach scores 1e6 times the median).  ``select="sample"``: the K candidates are DRAWN without replacement with probability
        ~ score^power / mean + c (engine.refine_keys: Gumbel top-k) instead of taken greedily -- the row rule stays: a candidate goes in only
        where its score is strictly larger than the row's.  With any of these the result also holds ``candidates``: the inserted points, host
        [replaced, 3]; ``candidate_indices`` are sample indices of the draw.  An array, select="top" and no exclude: exactly the calls above.
        Returns dict(replaced, rows, candidate_indices, score_replaced_max, score_inserted_min): how many rows changed, their row numbers in the
        whole set and the candidates that took their places (pairing order), the largest score that left and the smallest that came in (None
        when nothing was replaced).  Synchronises once (the indices come to the host).
        ``causal=True`` (int candidates only): the candidates' time column is drawn from the model's current causal table (resample_collocation,
        train(causal=...)) over the box's time range instead of the uniform law, so refinement and causal sampling compose instead of refinement
        pulling rows back to late times; without a table ValueError."""
        C = Candidates(self, candidates, 3, "(x, y, t)", select, power, c, seed, stream, box, exclude, causal)
        return refine_sharded_set(self, C, n_replace, self._score_weights(weights), ("x_c", "y_c", "t_c"))

    # ------------------------------------------------------------------------------------------
    # causal sampling of the collocation set's time coordinate (causal.py)
    # ------------------------------------------------------------------------------------------
    def residual_profile(self, bins, candidates, weights=None, *, exclude=(), seed=None):
        """(profile, counts), numpy [bins] each: the mean of residual_score per time bin of (lb_t, ub_t) over ``candidates`` probe points drawn
        uniformly in (lb, ub) on the device, and how many of them each bin holds; points inside the ``exclude`` discs (xc, yc, r) count in
        neither.  Four device calls (sample_box, residual_score, refine_keys in mask mode, binned_sums) and one download of 2 * bins doubles.
        The probe points are the same on every rank (stream 0x80000000 | round, ``round`` this model's count of device-drawn rounds), so with
        the same parameters every rank gets the same numbers bit for bit, no collective.  ``weights`` are the score's term weights, as in
        residual_score.  The causal weights and the table of a profile are not returned here: resample_collocation makes them from the same
        four calls plus causal_cdf and returns them as ``w`` and ``cdf``."""
        return causal_sampling.residual_profile(self, bins, candidates, weights, exclude=exclude, seed=seed)

    def resample_collocation(self, causal):
        """Causal sampling (Wang, Sankaran, Perdikaris): THIS RANK'S rows of the collocation set are drawn again with the time coordinate's
        density ~ max(w, floor), w_b = exp(-eps / ref * sum of the mean scores of the earlier time bins), the profile taken as in
        residual_profile.  ``causal``: dict(bins, eps, candidates, floor=0.0, exclude=(), seed=None, ref="first", weights=None, slack=None).
        ``ref="first"``: the mean score over the probe points of this model's FIRST profile (fetched once per model), which makes ``eps``
        dimensionless; a float is used as that scale.  The rows: N_shard + ``slack`` (default N_shard / 8 + 64) points from
        engine.sample_box(t_cdf=table) on the stream round * world + rank, the first N_shard of them outside the ``exclude`` discs go in; where
        fewer are valid the remaining rows keep their old points (no loop, no fallback draw).  N, the 1/N weights, the block boundaries and the
        shards stay; the host copies follow as in refine_collocation.  The device table stays as ``self._causal_cdf`` (refine_collocation(causal=True)
        draws from it).  Returns dict(redrawn, kept, w, cdf, profile, counts): rows drawn again and rows kept, the weights [bins], the table
        [bins + 1], the profile and the counts [bins] (numpy, downloaded here only -- train(causal=...) leaves them on the device)."""
        return causal_sampling.resample_collocation(self, causal, ("x_c", "y_c", "t_c"))

    # ------------------------------------------------------------------------------------------
    # identification of E, mu, rho: the moment sums of the collocation residuals (material.py)
    # ------------------------------------------------------------------------------------------
    def _material_weights(self, n_blk):
        """what _loss_and_grad puts on the seven collocation terms of a block of ``n_blk`` points"""
        return [self.layout["f_uv"] / n_blk] * 4 + [self.layout["f_s"] / n_blk] * 3

    def _material_rows(self):
        return self._n_collo

    def _material_engine_sums(self, lo, hi, **kw):
        s, e = self._shard(lo, hi)
        if e <= s:
            return None
        x, y, t = self._rows(lo, hi)
        return self.engine.material_sums(self.theta, x, y, t, self.lb, self.ub, self.normalize, self.E, self.mu, self.rho, True, **kw)

    def callback(self, loss):                        # INF:278-280, SEMI:285-288
        self.count = self.count + 1
        self.loss_rec.append(loss)
        if self.verbose and self.rank == 0:
            print('{} th iterations, Loss: {}'.format(self.count, loss))

    # ------------------------------------------------------------------------------------------
    # one evaluation of loss terms + total gradient on one collocation block
    # ------------------------------------------------------------------------------------------
    def _loss_and_grad(self, idx_start, idx_end, sums_out=None, adam=None):
        """Fills self._buf = [grad (P) | 8 floats per slot] with this rank's partial sums, then
        all-reduces.  Everything stays on the device.  Single process only: ``sums_out`` (a view of
        8*len(self.SLOTS) floats, zero where no set exists) receives the sums directly instead of the tail of the buffer.
        ``adam = (learning_rate, step)``: the caller wants the Adam update behind this gradient; where the whole evaluation is ONE library call
        (engine.wave_step: collocation set + side sets in one launch, one reduction) and no collective stands in between, the update rides in
        that reduction -- returns True then (the caller skips its own adam_step), False otherwise."""
        P, lay, eng, buf = self.n_params, self.layout, self.engine, self._buf
        n_blk = idx_end - idx_start
        s, e = self._shard(idx_start, idx_end)
        # slots this call's kernels (over)write: the collocation slot if this rank has rows of the block, every active non-empty side set
        writes = {0} if e > s else set()
        for k, name in enumerate(self.SLOTS[1:], start=1):
            if name in self._sides and lay[name] != 0.0 and self._sides[name][0].numel() > 0:
                writes.add(k)
        if sums_out is None or self._reduce:
            sums = buf[P:]
            # slots of skipped sets must read zero (getloss toggles the NB weight; a rank without rows of a set contributes nothing to the
            # reduced sum).  The kernels overwrite their slots, so only a slot that was written before and is NOT written now needs zeroing
            # -- in a training loop the same slots are written every step and no launch is spent here.
            stale = getattr(self, "_slots_dirty", set(range(len(self.SLOTS)))) - writes
            for k in stale:
                sums[8 * k:8 * k + 8].zero_()
            self._slots_dirty = set(writes)
            if self._reduce:
                # the all-reduce below leaves the GLOBAL total in every slot ANY rank wrote -- also in a slot this rank did not write
                # (a set or block with fewer rows than ranks: _shard gives e == s here).  Such a slot must be zeroed again before the next
                # collective, or the old total is added into it.  Which slots are written somewhere is a global fact (a side set is
                # registered on every rank with its global row count): mark them all.
                self._slots_dirty |= ({0} if n_blk > 0 else set()) | {k for k, name in enumerate(self.SLOTS[1:], start=1)
                                                                       if name in self._sides and lay[name] != 0.0}
        else:
            sums = sums_out
        grad = buf[:P]
        tw = [lay["f_uv"] / n_blk] * 4 + [lay["f_s"] / n_blk] * 3
        side = []
        for k, name in enumerate(_SLOTS[1:], start=1):
            if name not in self._sides or lay[name] == 0.0:
                continue
            x, y, t, tg, cols, n = self._sides[name]
            if x.numel() == 0:
                continue
            ow = [0.0] * 7
            for o in cols:
                ow[o] = lay[name] / n
            side.append((x, y, t, tg, ow, sums[8 * k:8 * k + 8]))
        # the traction set (slot "TRAC"): this rank's rows, if it has any -- a rank whose shard of the set is empty makes no call for it
        trac = None
        if "TRAC" in self._sides and lay["TRAC"] != 0.0 and self._sides["TRAC"][0].numel() > 0:
            x, y, t, aux, _, n = self._sides["TRAC"]
            k = self.SLOTS.index("TRAC")
            trac = (x, y, t, aux, [lay["TRAC"] / n] * 2, sums[8 * k:8 * k + 8])
        stepped = False
        if e > s and 1 <= len(side) + (trac is not None) <= 4 and hasattr(eng, "wave_step") and self._step_call:
            # the whole evaluation as ONE library call: repack | one persistent launch for all sets | one reduction (+ Adam); a traction set
            # takes one of the four slots of the one-stream part's set table (at most three value-only sets beside it)
            x, y, t = self._rows(idx_start, idx_end)
            fold = adam is not None and not self._reduce
            kw = {} if trac is None else {"traction": trac}
            eng.wave_step(self.theta, x, y, t, self.lb, self.ub, self.normalize, tw, side, grad, sums[0:8], self.E, self.mu, self.rho, True,
                          adam=(self.adam_m, self.adam_v, adam[0], adam[1]) if fold else None, **kw)
            stepped = fold
        else:
            wrote = False
            if e > s:
                x, y, t = self._rows(idx_start, idx_end)
                eng.wave_loss_grad(self.theta, x, y, t, self.lb, self.ub, self.normalize, tw, self.E, self.mu, self.rho, True,
                                   grad_out=grad, accumulate=False, loss_out=sums[0:8])
                wrote = True
            for i in range(0, len(side), 4):           # all value-only sets of the step in one call (up to PINN_MAX_SETS per call)
                eng.data_loss_grad_multi(self.theta, side[i:i + 4], self.lb, self.ub, self.normalize, grad_out=grad, accumulate=wrote, packed=wrote)
                wrote = True
            if trac is not None:                       # (Adam never runs before this gradient is in: the caller's adam_step follows)
                eng.wave_traction_loss_grad(self.theta, trac[0], trac[1], trac[2], self.lb, self.ub, self.normalize, trac[3], trac[4],
                                            grad_out=grad, accumulate=wrote, loss_out=trac[5], packed=wrote)
                wrote = True
            if not wrote:
                grad.zero_()
        if self._reduce:
            # one fused buffer [gradient | loss sums] (latency-bound message); enqueued behind the kernels in stream order, and Adam is
            # enqueued behind it: the host never waits
            fold = adam is not None and self._p2p is not None
            stepped = all_reduce_sum(buf, self.pg, getattr(self, "collective_events", None), self._p2p,
                                     (self.theta, self.adam_m, self.adam_v, adam[0], adam[1]) if fold else None, P)
        return stepped

    # ------------------------------------------------------------------------------------------
    # training drivers
    # ------------------------------------------------------------------------------------------
    def train(self, iter, learning_rate, batch_num, record="pre", refine=None, validate=None, identify=None, causal=None):
        """Adam loop of INF:282-319: contiguous collocation blocks, ``iter`` steps per block, all
        side sets fed whole to every block.  Returns the per-step lists
        (loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss); with a traction set (TRAC=...) its per-step term is appended to ``self.trac_rec``, and with at
        most three value-only sets beside it the step is still ONE library call: the set rides in the step launch's one-stream part
        (pinn_wave2d_step_traction) -- measured on an MI355X at 8x64, f16x3, 2 M collocation + IC 10 201 + SRC 70 400 points: 4.376 ms per
        step without the set, 4.389 ms with 20 000 traction points, 4.522 ms with step_call=False (profiles/wave_traction_calls.txt).  ``record="pre"`` (default): each recorded value is the loss
        the step's gradient was taken at -- free.  ``record="post"``: the reference's own bookkeeping, every term re-evaluated
        AFTER the update (its four to six extra sess.run calls per step, INF:308-317) -- one more loss+gradient evaluation per step.
        ``refine``: None, or dict(every, candidates, n_replace, ...) -- refine_collocation with that many device-drawn candidates behind every
        ``every``-th step of this call (refine.RefineSchedule; the further entries are refine_collocation's keywords).
        ``validate``: None, or dict(every, points=(x, y, t), ref={name: column}, fields=(...)) -- the relative L2 of predict's fields against
        ``ref`` behind every ``every``-th step (validate.ValidateSchedule): the sums stay on the device until the block's host synchronisation,
        the results are appended to ``self.val_rec`` as (step, dict).
        ``identify``: None, or dict(params=("E", "mu"), lr=1e-3, every=1, bounds=dict(mu=(0.0, 0.49))) -- the named constants (any of E, mu,
        rho) are identified while the net trains (material.MaterialSchedule): behind every ``every``-th step one forward-only call takes the
        fp64 moment sums of the step's collocation block at the step's weights, and a float64 Adam on the host (log E, mu, log rho) moves the
        constants; the next step's call sees them.  (step, E, mu, rho) is appended to ``self.material_rec``.  Cost: one more forward pass
        over the block per identified step -- measured on an MI355X at 8x64, f16x3, 2 M points: 4.61 ms per step with None, 7.09 ms with
        every=1, 5.24 ms with every=4 (profiles/material_sums_calls.txt); choose ``every`` accordingly.  With None the loop makes exactly the
        calls it makes without the keyword.
        ``causal``: None, or dict(every, bins, eps, candidates, floor=0.0, exclude=(), seed=None, ref="first") -- resample_collocation's entries
        plus ``every``: behind every ``every``-th step of this call, in front of refinement's hook, the time profile of the residual score is
        taken on the device and this rank's rows are drawn again from its causal table (causal.CausalSchedule).  Every trigger redraws, the
        first one of a fresh model too: with ``ref="first"`` and no scale yet it fetches its own profile (2 * bins doubles, once per model)
        and takes the scale from it.  Otherwise the profile, the weights and the table stay on the device.  Each trigger is ONE HOST
        SYNCHRONISATION, as a refinement round is: the count of valid drawn points and the redrawn rows (N_shard points, 12 bytes each) come
        to the host for the host copies of the set, and the float64 columns are rewritten (26 - 49 ms per trigger at 2 M rows); choose
        ``every`` so that this is small beside ``every`` steps.  Measured on an MI355X at 8x64, f16x3, 2 M points: 4.45 - 4.48 ms per step
        with None (the code before the keyword: 4.46 - 4.49), 4.78 - 4.93 ms with every=100, 65 536 probe points and the default scale
        (4.74 - 4.83 with a given one; profiles/causal_calls.txt).  With None the loop makes exactly the calls it makes without the keyword."""
        if record not in ("pre", "post"):
            raise ValueError("record must be 'pre' or 'post'")
        sched, vsched, msched, step = schedule(self, refine), validate_schedule(self, validate), material.schedule(self, identify), 0
        csched = causal_sampling.schedule(self, causal, ("x_c", "y_c", "t_c"))
        loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss = [], [], [], [], []
        P = self.n_params
        col_num = self._n_collo
        for i in range(batch_num):
            idx_start = int(i * col_num / batch_num)
            idx_end = int((i + 1) * col_num / batch_num)
            rec = torch.zeros((iter, 8 * len(self.SLOTS)), dtype=torch.float32, device=self.device)

            def probe():
                self._loss_and_grad(idx_start, idx_end)
                return self._buf

            if iter > 0:
                self._settle_adjoint_shift(self.engine, probe, P)
            for it in range(iter):
                self.adam_t += 1
                if msched is not None:
                    # (the workspace holds the packed form of the current weights only behind a record="post" re-evaluation)
                    msched.before_step(step + 1, idx_start, idx_end, packed=record == "post" and step > 0)
                updated = self._loss_and_grad(idx_start, idx_end, sums_out=rec[it], adam=(learning_rate, self.adam_t))     # (sums_out: one launch less per step than copying afterwards)
                if self._reduce:
                    rec[it].copy_(self._buf[P:])
                if not updated:
                    self.engine.adam_step(self.theta, self.adam_m, self.adam_v, self._buf[:P], learning_rate, self.adam_t)
                if record == "post":                 # INF:308-317: the terms at the updated weights
                    self._loss_and_grad(idx_start, idx_end)
                    rec[it].copy_(self._buf[P:])
                if self.verbose and it % 10 == 0 and self.rank == 0:
                    tm = self._terms_from_sums(rec[it].detach().cpu().numpy().reshape(len(self.SLOTS), 8), idx_end - idx_start)
                    print('It: %d, Loss: %.3e' % (it, tm["loss"]))
                if sched is not None or vsched is not None or msched is not None or csched is not None:
                    step += 1
                    if msched is not None:
                        msched.after_step()
                    if csched is not None:
                        csched.after_step(step)
                    if sched is not None:
                        sched.after_step(step)
                    if vsched is not None:
                        vsched.after_step(step)
            sums = rec.detach().cpu().numpy().reshape(iter, len(self.SLOTS), 8)
            if vsched is not None:
                vsched.flush()
            self._check_collective()                 # (behind the block's one host synchronisation)
            if iter > 0 and not bool(torch.isfinite(self.theta).all()):
                raise FloatingPointError("parameters became non-finite during train(): residuals outgrew the 16-bit reverse pass; "
                                         "lower the learning rate or raise engine.adjoint_shift")
            for it in range(iter):
                tm = self._terms_from_sums(sums[it], idx_end - idx_start)
                loss_f_uv.append(tm["loss_f_uv"])
                loss_f_s.append(tm["loss_f_s"])
                loss_IC.append(tm["loss_IC"])
                loss_SRC.append(tm["loss_SRC"])
                loss.append(tm["loss"])
                if "loss_TRAC" in tm:
                    self.trac_rec.append(tm["loss_TRAC"])
        return loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss

    def train_bfgs(self, batch_num, options: Optional[dict] = None, backend: str = "scipy"):
        """L-BFGS-B stage of INF:321-335: scipy on the host over a float64 copy of the flat
        parameter vector, loss and gradient from the device kernels; ``callback`` fires once per
        function evaluation like ScipyOptimizerInterface's loss_callback.  ``backend="torch"``: the same stage with the
        optimizer on the device as well (lbfgs_on_device), for when the host update is the bottleneck.  ``backend="hip"``: the library's own
        L-BFGS (lbfgs_hip): no host round trip per evaluation, the callbacks arrive in batches.  Any other name raises ValueError.
        The material constants stay where they are: identification (train(identify=...)) belongs to the Adam loop only."""
        check_backend(backend)
        opts = dict(BFGS_OPTIONS[self.case])
        if options:
            opts.update(options)
        col_num = self._n_collo
        result = None
        for i in range(batch_num):
            idx_start = int(i * col_num / batch_num)
            idx_end = int((i + 1) * col_num / batch_num)

            def evaluate():
                self._loss_and_grad(idx_start, idx_end)
                return self._buf

            result = self._lbfgs_stage(backend, self.engine, self.theta, evaluate,
                                       lambda sums: self._terms_from_sums(sums.reshape(len(self.SLOTS), 8), idx_end - idx_start)["loss"],
                                       self._loss_coeffs(idx_end - idx_start), opts)
        return result

    # ------------------------------------------------------------------------------------------
    # inference / diagnostics
    # ------------------------------------------------------------------------------------------
    def predict(self, x_star, y_star, t_star):
        """INF:337-347: (u, v, s11, s22, s12, e11, e22, e12), each numpy [M,1]."""
        F = self._fields(x_star, y_star, t_star)
        out = torch.stack([F[0, 0], F[0, 1], F[0, 4], F[0, 5], F[0, 6], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]])
        return self._cols(out)

    probe = predict                                  # INF:349-359 is a verbatim copy of predict

    # predict on the device (validate.PredictMixin: predict_device, predict_frames, validate): the predict head carries value, d/dx, d/dy only
    PREDICT_FIELDS = ("u", "v", "s11", "s22", "s12", "e11", "e22", "e12")
    PREDICT_INPUTS = ("x", "y", "t")
    VALIDATE_FIELDS = ("u", "v", "s11", "s22", "s12")             # what FEM frames carry (pointsets.preprocess)

    def _predict_engine(self):
        return self.engine

    def _predict_cols(self, xs):
        return self.engine.wave_predict(self.theta, xs[0], xs[1], xs[2], self.lb, self.ub, self.normalize)

    def getloss(self):
        """INF:361-376: (loss, loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss_NB) on the full sets."""
        n = self._n_collo
        self._loss_and_grad(0, n)
        host = self._buf[self.n_params:].detach().cpu().numpy().reshape(len(self.SLOTS), 8)
        self._check_collective()
        tm = self._terms_from_sums(host, n)
        if self.layout["NB"] == 0.0 and "NB" in self._sides:
            # loss_NB is reported by getloss even where it is excluded from the total (INF:117-119,374)
            lay = dict(self.layout)
            self.layout = dict(lay, NB=1.0)
            try:
                self._loss_and_grad(0, n)
                h2 = self._buf[self.n_params:].detach().cpu().numpy().reshape(len(self.SLOTS), 8)
                tm["loss_NB"] = self._terms_from_sums(h2, n)["loss_NB"]
            finally:
                self.layout = lay
        return tm["loss"], tm["loss_f_uv"], tm["loss_f_s"], tm["loss_IC"], tm["loss_SRC"], tm["loss_NB"]

    def getloss_dict(self):
        """Every loss term on the full sets by name: loss, loss_f_uv, loss_f_s and loss_<set> of each slot (loss_TRAC with a traction set); the
        terms as they enter the total -- a set the layout excludes reads 0 here where getloss re-evaluates loss_NB."""
        n = self._n_collo
        self._loss_and_grad(0, n)
        host = self._buf[self.n_params:].detach().cpu().numpy().reshape(len(self.SLOTS), 8)
        self._check_collective()
        return self._terms_from_sums(host, n)


class DeepHPMConfined(DeepHPM):
    """Signature of the confined-domain script (CONF:23): its distance/particular networks are
    created but never enter the graph there (CONF:282-294 ignores them), so they are accepted,
    initialised (so that save_NN can write them, CONF:197-217) and otherwise ignored here too."""

    def __init__(self, Collo, SRC, IC, FIXED, DIST, uv_layers, dist_layers, part_layers, lb, ub,
                 uvDir='', partDir='', distDir='', **kw):
        super().__init__(Collo, SRC, IC, None, uv_layers, lb, ub, ExistModel=1 if uvDir else 0, modelDir=uvDir,
                         case="confined", FIX=FIXED, **kw)
        self.DIST = DIST
        self.dist_layers = None if dist_layers is None else [int(v) for v in dist_layers]
        self.part_layers = None if part_layers is None else [int(v) for v in part_layers]
        seed = kw.get("seed", 1111)
        self._aux_nets = {}
        for name, layers, path, off in (("DIST", self.dist_layers, distDir, 1), ("PART", self.part_layers, partDir, 2)):
            if layers is not None:
                self._aux_nets[name] = self.load_NN(path, layers) if path else xavier_init(layers, np.random.default_rng(seed + off))

    def train(self, iter, learning_rate, batch_num, record="pre", refine=None, validate=None, identify=None, causal=None):
        """CONF:373-408 returns three lists: (loss_f_uv, loss_f_s, loss)."""
        loss_f_uv, loss_f_s, _, _, loss = super().train(iter, learning_rate, batch_num, record, refine, validate, identify, causal)
        return loss_f_uv, loss_f_s, loss

    def save_NN(self, fileDir, TYPE=''):
        """CONF:197-217: TYPE selects the net ('UV', 'DIST', 'PART'); anything else writes nothing."""
        if TYPE in ('UV', ''):
            return super().save_NN(fileDir)
        if TYPE in ('DIST', 'PART') and TYPE in self._aux_nets:
            W, b = self._aux_nets[TYPE]
            write_checkpoint(fileDir, W, b, self.dist_layers if TYPE == 'DIST' else self.part_layers)
            if self.verbose:
                print("Save %s NN parameters successfully..." % TYPE)

    def getloss(self):
        """CONF:453-472: (loss, loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss_FIX) on the full sets."""
        n = self._n_collo
        self._loss_and_grad(0, n)
        host = self._buf[self.n_params:].detach().cpu().numpy().reshape(len(self.SLOTS), 8)
        self._check_collective()
        tm = self._terms_from_sums(host, n)
        return tm["loss"], tm["loss_f_uv"], tm["loss_f_s"], tm["loss_IC"], tm["loss_SRC"], tm["loss_FIX"]
