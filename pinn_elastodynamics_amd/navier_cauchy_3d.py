"""3-D Navier-Cauchy half-space model (BASELINE.json configs[4]) -- a BUILD-SIDE EXTENSION, not in the reference.

The reference's four scripts are 2-D + time.  This class carries their model-class surface
(``class DeepHPM``, ElasticWaveSemiInfinite/ElasticWave.py = SEMI) over to four inputs (x, y, z, t) and twelve outputs
(u, v, w, ut, vt, wt, s11, s22, s33, s12, s13, s23): same method names and column-tensor convention, the mixed-variable
formulation of SEMI:228-272 written for three dimensions (stated term by term in include/pinn_hip.h and DESIGN.md), the loss layout of
SEMI:112-127 with the traction-free top surface as the ``loss_NB`` term.  Kernels: pinn_nc3d_* of include/pinn_hip.h.
Parity for this case is unpinned by definition (there is nothing in the reference to compare with).

Data parallel exactly like the 2-D classes: every point set is sharded into contiguous row ranges (a rank uploads only its own
rows), partial sums carry the global 1/N, one all-reduce of [gradient | loss sums], identical on-device Adam on every rank.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import material
from .model_base import ShardedSetsModel
from .optim import all_reduce_sum, check_backend
from .refine import Candidates, refine_sharded_set, schedule, score_weights

OUT = ("u", "v", "w", "ut", "vt", "wt", "s11", "s22", "s33", "s12", "s13", "s23")
_SLOTS = ("collo", "IC", "SRC", "NB")          # 16 floats each in the loss-sum buffer
LOSS_LAYOUT_3D = dict(f_uv=5.0, f_s=5.0, IC=2.0, SRC=2.0, NB=2.0)        # the semi-infinite script's weights (SEMI:127)


class NavierCauchy3D(ShardedSetsModel, material.MaterialMixin):
    """NavierCauchy3D(Collo[N,4], SRC[Ns,7], IC[Ni,4], TOP[Nt,4], uv_layers, lb[4], ub[4], ExistModel=0, modelDir='')

    Collo: collocation points (x, y, z, t); SRC: points with prescribed displacement (x, y, z, t, u, v, w) -- the source;
    IC: points at t = 0 where u, v, w, ut, vt, wt vanish; TOP: points on the free surface z = ub[2] where s33 = s13 = s23 = 0.
    uv_layers = [4] + depth * [width] + [12]."""
    N_IN, COLLO_NAMES = 4, ("x_c", "y_c", "z_c", "t_c")
    COLLO_TERMS, SUMS_STRIDE, SLOTS = (6, 6), 16, _SLOTS
    material_family = material.NC3D

    def __init__(self, Collo, SRC, IC, TOP, uv_layers, lb, ub, ExistModel=0, modelDir='', *, precision="f16x3", engine=None, seed=1111,
                 process_group=None, verbose=True, E=2.5, mu=0.25, rho=1.0, normalize=True, layout: Optional[dict] = None,
                 always_reduce=False, collective="rccl", p2p_timeout_s=None):
        self.count = 0
        self._shift_state = {}
        self.loss_rec = []
        self.layout = dict(LOSS_LAYOUT_3D if layout is None else layout)
        self.normalize = bool(normalize)
        self.lb = np.asarray(lb, dtype=np.float64).reshape(-1)
        self.ub = np.asarray(ub, dtype=np.float64).reshape(-1)
        assert self.lb.size == 4 and self.ub.size == 4, "lb / ub are (x, y, z, t) bounds"
        self.E, self.mu, self.rho = E, mu, rho
        self.uv_layers = [int(v) for v in uv_layers]
        assert self.uv_layers[0] == 4 and self.uv_layers[-1] == 12, "uv_layers = [4] + depth*[width] + [12]"
        self.verbose = verbose
        self._init_topology(process_group, always_reduce)
        self._set_engine(self._default_engine(self.uv_layers, precision, np.asarray(Collo).shape[0]) if engine is None else engine, "nc3d")
        self._init_net(seed, ExistModel, modelDir)
        self._init_collocation(Collo)
        self._add_side("IC", IC, (0, 1, 2, 3, 4, 5))                 # u, v, w, ut, vt, wt = 0 at t = 0      (as SEMI:119-122)
        self._add_side("SRC", SRC, (0, 1, 2), (4, 5, 6))             # prescribed source displacement       (as SEMI:123-124)
        self._add_side("NB", TOP, (8, 10, 11))                       # s33 = s13 = s23 = 0 on the free top  (as SEMI:125-126)
        self.SRC, self.IC, self.TOP = SRC, IC, TOP
        self._buf = torch.zeros(self.n_params + 16 * len(_SLOTS), dtype=torch.float32, device=self.device)
        self._init_collective(collective, p2p_timeout_s)

    # ---- graph pieces on column arrays [N,1] ---------------------------------------------------------------------------
    def _fields(self, x, y, z, t):
        xs = self._device_columns((x, y, z, t))
        return self.engine.nc3d_fields(self.theta, *xs, self.lb, self.ub, self.normalize)        # [5, 12, N]

    # neural_net(X, weights, biases): net_api.NetApi, through _current_theta and this
    def _net_fields(self, eng, theta, X):
        xs = self._device_columns((X[:, k] for k in range(4)), eng.device)
        return eng.nc3d_fields(theta, *xs, self.lb, self.ub, self.normalize)[0]

    def net_uv(self, x, y, z, t):
        """-> (u, v, w, ut, vt, wt, s11, s22, s33, s12, s13, s23), each [N,1]"""
        return self._cols(self._fields(x, y, z, t)[0])

    def net_e(self, x, y, z, t):
        """-> (e11, e22, e33, e12, e13, e23), engineering shear as INF:216-218"""
        F = self._fields(x, y, z, t)
        X, Y, Z = F[1], F[2], F[3]
        return self._cols(torch.stack([X[0], Y[1], Z[2], Y[0] + X[1], Z[0] + X[2], Z[1] + Y[2]]))

    def net_f_sig(self, x, y, z, t):
        """-> the twelve residuals (f_u, f_v, f_w, f_ut, f_vt, f_wt, f_s11, f_s22, f_s33, f_s12, f_s13, f_s23)"""
        F = self._fields(x, y, z, t)
        V, X, Y, Z, T = F[0], F[1], F[2], F[3], F[4]
        E, mu, rho = self.E, self.mu, self.rho
        coef = E / ((1 + mu) * (1 - 2 * mu))
        c1, c2, G = coef * (1 - mu), coef * mu, E / (2 * (1 + mu))
        e11, e22, e33 = X[0], Y[1], Z[2]
        e12, e13, e23 = Y[0] + X[1], Z[0] + X[2], Z[1] + Y[2]
        f = [X[6] + Y[9] + Z[10] - rho * T[3], X[9] + Y[7] + Z[11] - rho * T[4], X[10] + Y[11] + Z[8] - rho * T[5],
             T[0] - V[3], T[1] - V[4], T[2] - V[5],
             V[6] - (c1 * e11 + c2 * (e22 + e33)), V[7] - (c1 * e22 + c2 * (e11 + e33)), V[8] - (c1 * e33 + c2 * (e11 + e22)),
             V[9] - G * e12, V[10] - G * e13, V[11] - G * e23]
        return self._cols(torch.stack(f))

    net_uvp = net_uv
    net_f = net_f_sig

    # ---- residual-adaptive refinement of the collocation set (refine.py) ----------------------------------------------
    def _score_weights(self, weights):
        """the coefficients the loss layout puts on the twelve collocation terms, unless the caller gives twelve of its own"""
        return score_weights(weights, [self.layout["f_uv"]] * 6 + [self.layout["f_s"]] * 6,
                             "(f_u, f_v, f_w, f_ut, f_vt, f_wt, f_s11, f_s22, f_s33, f_s12, f_s13, f_s23)")

    def _score_device(self, xs, w, packed=False):
        kw = {"packed": True} if packed else {}
        return self.engine.nc3d_residual_score(self.theta, xs[0], xs[1], xs[2], xs[3], self.lb, self.ub, self.normalize, w, self.E, self.mu,
                                               self.rho, **kw)

    def residual_score(self, x, y, z, t, weights=None):
        """sum_i weights[i] * f_i^2 of net_f_sig's twelve residuals per point, numpy [N,1], formed on the device: the measure
        refine_collocation ranks by.  Default ``weights``: what the loss layout puts on the collocation terms."""
        xs = self._device_columns((x, y, z, t))
        return self._score_device(xs, self._score_weights(weights)).detach().cpu().numpy().reshape(-1, 1)

    def refine_collocation(self, candidates, n_replace, weights=None, *, select="top", power=1.0, c=1.0, seed=None, stream=None, box=None, exclude=()):
        """Residual-adaptive refinement that keeps the set's size, exactly as elastic_wave.DeepHPM.refine_collocation with four columns:
        ``candidates`` [Nc,4] (x, y, z, t); the K = min(n_replace, Nc, rows) lowest-scoring rows of this rank give way to the K highest-scoring
        candidates where those score strictly higher.  N, the 1/N weights, the block boundaries of train(batch_num), the workspace and the
        shards stay; the host copies (x_c, y_c, z_c, t_c) follow on copies.  Data parallel: no collective, pass rank-distinct candidates.
        ``candidates`` may be an INT: that many points are drawn on the device in ``box`` = (lo, hi), default (lb, ub), by
        engine.sample_box(seed, stream) -- counter-based, so the points are a function of (seed, stream, index) alone; ``stream`` defaults to
        round * world + rank, ``round`` counting this model's device-drawn refinements: ranks and rounds get distinct, reproducible candidates
        with no coordination.  ``exclude``: discs (xc, yc, r) -- cylinders along z -- or balls (xc, yc, zc, r) whose inside and boundary never enter the set (the source disc, a hole: single
        points there reach scores 1e6 times the median).  ``select="sample"``: the K candidates are DRAWN without replacement with probability
        ~ score^power / mean + c (engine.refine_keys: Gumbel top-k) instead of taken greedily -- the row rule stays: a candidate goes in only
        where its score is strictly larger than the row's.  With any of these the result also holds ``candidates``: the inserted points, host
        [replaced, 4]; ``candidate_indices`` are sample indices of the draw.  An array, select="top" and no exclude: exactly the calls above.
        Returns dict(replaced, rows, candidate_indices, score_replaced_max, score_inserted_min).  Synchronises once."""
        C = Candidates(self, candidates, 4, "(x, y, z, t)", select, power, c, seed, stream, box, exclude)
        return refine_sharded_set(self, C, n_replace, self._score_weights(weights), ("x_c", "y_c", "z_c", "t_c"))

    # ---- identification of E, mu, rho: the moment sums of the collocation residuals (material.py) ----------------------
    def _material_weights(self, n_blk):
        """what _loss_and_grad puts on the twelve collocation terms of a block of ``n_blk`` points"""
        return [self.layout["f_uv"] / n_blk] * 6 + [self.layout["f_s"] / n_blk] * 6

    def _material_rows(self):
        return self._n_collo

    def _material_engine_sums(self, lo, hi, **kw):
        s, e = self._shard(lo, hi)
        if e <= s:
            return None
        x, y, z, t = self._rows(lo, hi)
        return self.engine.nc3d_material_sums(self.theta, x, y, z, t, self.lb, self.ub, self.normalize, self.E, self.mu, self.rho, **kw)

    def callback(self, loss):
        self.count += 1
        self.loss_rec.append(loss)
        if self.verbose and self.rank == 0:
            print('{} th iterations, Loss: {}'.format(self.count, loss))

    # ---- loss + gradient of one collocation block -----------------------------------------------------------------------
    def _loss_and_grad(self, idx_start, idx_end):
        """self._buf = [grad (P) | 16 floats per slot], this rank's partial sums, then all-reduced."""
        P, lay, eng, buf = self.n_params, self.layout, self.engine, self._buf
        sums = buf[P:]
        sums.zero_()
        grad = buf[:P]
        n_blk = idx_end - idx_start
        s, e = self._shard(idx_start, idx_end)
        tw = [lay["f_uv"] / n_blk] * 6 + [lay["f_s"] / n_blk] * 6
        wrote = False
        if e > s:
            x, y, z, t = self._rows(idx_start, idx_end)
            eng.nc3d_loss_grad(self.theta, x, y, z, t, self.lb, self.ub, self.normalize, tw, self.E, self.mu, self.rho,
                               grad_out=grad, accumulate=False, loss_out=sums[0:16])
            wrote = True
        for k, name in enumerate(_SLOTS[1:], start=1):
            if name not in self._sides or lay[name] == 0.0:
                continue
            x, y, z, t, tg, cols, n = self._sides[name]
            if x.numel() == 0:
                continue
            ow = [0.0] * 12
            for o in cols:
                ow[o] = lay[name] / n
            eng.nc3d_data_loss_grad(self.theta, x, y, z, t, self.lb, self.ub, self.normalize, tg, ow, grad_out=grad, accumulate=wrote,
                                    loss_out=sums[16 * k:16 * k + 16], packed=wrote)
            wrote = True
        if not wrote:
            grad.zero_()
        if self._reduce:
            all_reduce_sum(buf, self.pg, getattr(self, "collective_events", None), getattr(self, "_p2p", None))

    # ---- training drivers ---------------------------------------------------------------------------------------------
    def train(self, iter, learning_rate, batch_num, refine=None, identify=None):
        """Adam loop with the reference's block-sequential batching (SEMI:290-328): returns the per-step lists
        (loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss) -- the loss each step's gradient was taken at.  ``refine``: None, or
        dict(every, candidates, n_replace, ...): refine_collocation with device-drawn candidates behind every ``every``-th step of this call.
        ``identify``: None, or dict(params=("E", "mu"), lr=1e-3, every=1, bounds=...) as in elastic_wave.DeepHPM.train: behind every
        ``every``-th step one forward-only call takes the 24 fp64 sums of the step's block (pinn_nc3d_material_sums) at the step's weights
        and constants, a float64 Adam on the host moves the named constants, (step, E, mu, rho) is appended to ``self.material_rec``.  Cost,
        MI355X, 10x128, f16x3, 200 000 points: 4.85 ms per step with None, 5.97 with every=1, 5.10 with every=4
        (profiles/material_family_calls.txt).  With None the loop makes exactly the calls it makes without the keyword."""
        P, L = self.n_params, len(_SLOTS)
        sched, msched, step = schedule(self, refine), material.schedule(self, identify), 0
        hist = ([], [], [], [], [])
        for i in range(batch_num):
            lo, hi = int(i * self._n_collo / batch_num), int((i + 1) * self._n_collo / batch_num)
            rec = torch.zeros((iter, 16 * L), dtype=torch.float32, device=self.device)

            def probe():
                self._loss_and_grad(lo, hi)
                return self._buf

            if iter > 0:
                self._settle_adjoint_shift(self.engine, probe, P)
            for it in range(iter):
                if msched is not None:
                    msched.before_step(step + 1, lo, hi)
                self._loss_and_grad(lo, hi)
                rec[it].copy_(self._buf[P:])
                self.adam_t += 1
                self.engine.adam_step(self.theta, self.adam_m, self.adam_v, self._buf[:P], learning_rate, self.adam_t)
                if sched is not None or msched is not None:
                    step += 1
                    if msched is not None:
                        msched.after_step()
                    if sched is not None:
                        sched.after_step(step)
            sums = rec.detach().cpu().numpy().reshape(iter, L, 16)
            self._check_collective()                 # (behind the block's one host synchronisation)
            if iter > 0 and not bool(torch.isfinite(self.theta).all()):
                raise FloatingPointError("parameters became non-finite during train(): lower the learning rate or raise engine.adjoint_shift")
            for it in range(iter):
                tm = self._terms_from_sums(sums[it], hi - lo)
                for lst, key in zip(hist, ("loss_f_uv", "loss_f_s", "loss_IC", "loss_SRC", "loss")):
                    lst.append(tm[key])
        return hist

    def train_bfgs(self, batch_num, options: Optional[dict] = None, backend: str = "scipy"):
        """L-BFGS stage on the device kernels, as SEMI:330-344.  ``backend="scipy"`` (default): scipy's L-BFGS-B on the host over a float64
        copy of the flat vector; ``"torch"``: torch.optim.LBFGS on the device (optim.lbfgs_on_device); ``"hip"``: the library's own
        L-BFGS, no host round trip per evaluation (optim.lbfgs_hip: the callbacks arrive in batches).  Any other name raises ValueError.
        The material constants stay where they are: identification (train(identify=...)) belongs to the Adam loop only."""
        check_backend(backend)
        L = len(_SLOTS)
        opts = dict(maxiter=1000, maxfun=1000, maxcor=50, maxls=50, ftol=0.001 * float(np.finfo(float).eps))       # SEMI:130-137
        if options:
            opts.update(options)
        result = None
        for i in range(batch_num):
            lo, hi = int(i * self._n_collo / batch_num), int((i + 1) * self._n_collo / batch_num)

            def evaluate():
                self._loss_and_grad(lo, hi)
                return self._buf

            result = self._lbfgs_stage(backend, self.engine, self.theta, evaluate,
                                       lambda sums: self._terms_from_sums(sums.reshape(L, 16), hi - lo)["loss"], self._loss_coeffs(hi - lo), opts)
        return result

    # ---- inference / diagnostics ---------------------------------------------------------------------------------------
    def predict(self, x_star, y_star, z_star, t_star):
        """-> (u, v, w, s11, s22, s33, s12, s13, s23, e11, e22, e33, e12, e13, e23), each numpy [M,1] (the 3-D form of INF:337-347)"""
        F = self._fields(x_star, y_star, z_star, t_star)
        V, X, Y, Z = F[0], F[1], F[2], F[3]
        return self._cols(torch.stack([V[0], V[1], V[2], V[6], V[7], V[8], V[9], V[10], V[11],
                                       X[0], Y[1], Z[2], Y[0] + X[1], Z[0] + X[2], Z[1] + Y[2]]))

    probe = predict

    def getloss(self):
        """(loss, loss_f_uv, loss_f_s, loss_IC, loss_SRC, loss_NB) on the full sets (as SEMI:370-385)"""
        self._loss_and_grad(0, self._n_collo)
        tm = self._terms_from_sums(self._buf[self.n_params:].detach().cpu().numpy().reshape(len(_SLOTS), 16), self._n_collo)
        self._check_collective()
        return tm["loss"], tm["loss_f_uv"], tm["loss_f_s"], tm["loss_IC"], tm["loss_SRC"], tm["loss_NB"]


def halfspace_case(n_collo=100_000, n_ic=8000, n_top=8000, n_src=(60, 60), seed=1111, width=128, depth=10,
                   lb=(0.0, 0.0, -30.0, 0.0), ub=(30.0, 30.0, 0.0, 15.0), src_center=(15.0, 15.0, -8.0), src_r=2.0):
    """Seeded point sets of a half space z <= 0 with a buried spherical source driven by a Ricker pulse (the 3-D analogue of
    SEMI:667-769): collocation points in the box minus the source sphere, an initial-state set at t = 0, a traction-free set on
    z = 0, and the source surface at n_src[1] times.  Returns a dict with Collo, IC, TOP, SRC, uv_layers, lb, ub."""
    rng = np.random.default_rng(seed)
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    c = np.asarray(src_center, dtype=np.float64)

    def lhs(n, d):
        return np.stack([(rng.permutation(n) + rng.random(n)) / n for _ in range(d)], axis=1)

    out = np.zeros((0, 4))
    while out.shape[0] < n_collo:
        P = lb + (ub - lb) * lhs(int((n_collo - out.shape[0]) * 1.05) + 64, 4)
        out = np.concatenate([out, P[((P[:, :3] - c) ** 2).sum(1) > src_r ** 2]], 0)
    Collo = out[:n_collo]
    IC = lb + (ub - lb) * lhs(n_ic, 4)
    IC[:, 3] = 0.0
    IC = IC[((IC[:, :3] - c) ** 2).sum(1) > src_r ** 2]
    TOP = lb + (ub - lb) * lhs(n_top, 4)
    TOP[:, 2] = ub[2]
    n_pt, n_time = n_src
    # quasi-uniform points on the sphere (Fibonacci lattice), Ricker amplitude as INF:691-704, radial displacement
    k = np.arange(n_pt) + 0.5
    phi, th = np.arccos(1 - 2 * k / n_pt), np.pi * (1 + 5 ** 0.5) * k
    nrm = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    tt = np.linspace(0.0, ub[3], n_time + 1)[1:]
    amp = (2 * np.pi ** 2 * (tt - 3.0) ** 2 / 9.0 - 1) * np.exp(-np.pi ** 2 * (tt - 3.0) ** 2 / 9.0)
    pts = np.repeat((c + src_r * nrm)[None], n_time, 0).reshape(-1, 3)
    tcol = np.repeat(tt, n_pt)
    disp = (amp[:, None, None] * nrm[None]).reshape(-1, 3)
    SRC = np.concatenate([pts, tcol[:, None], disp], 1)
    return dict(Collo=Collo, IC=IC, TOP=TOP, SRC=SRC, uv_layers=[4] + depth * [width] + [12], lb=lb, ub=ub, source=(c, src_r))
