"""Host-side mirror of the reference's plate-with-hole model class (PLATE = PlateHoleQuarter/train/train.py).

``PINN(Collo, HOLE, IC, LF, RT, UP, LW, DIST, uv_layers, dist_layers, part_layers, lb, ub, partDir, distDir, uvDir)`` keeps
the reference's constructor (PLATE:28-29), method names and the ``[N,1]`` column convention: three nets (uv, distance,
particular), composite fields ``P + D*N`` (PLATE:358-388), the three-stage schedule ``train_bfgs_dist`` ->
``train_bfgs_part`` -> ``train`` / ``train_bfgs`` (PLATE:953-972), ``predict`` / ``predict_D`` / ``predict_P`` / ``getloss``
and ``save_NN(fileDir, TYPE)`` / ``load_NN``.  All loss / gradient work runs in the HIP kernels behind include/pinn_hip.h
(5-stream family: value, d/dx, d/dy, d/dt, d2/dt2); the streams of the frozen distance and particular nets on the
collocation and hole points are computed once and kept on the device, because those nets do not change while the uv net
trains (PLATE:240-241).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .model_base import ModelBase
from .optim import all_reduce_sum, check_backend, device_array, lbfgs_hip, lbfgs_on_device, pack_params
from . import material
from .refine import Candidates, empty_result, schedule, score_weights, select_pairs, update_host_columns
from .validate import PredictMixin, schedule as validate_schedule

_EPS = float(np.finfo(float).eps)
BFGS_OPTIONS = {   # PLATE:220-247
    "dist": dict(maxiter=20000, maxfun=20000, maxcor=50, maxls=50, ftol=0.00001 * _EPS),
    "part": dict(maxiter=20000, maxfun=20000, maxcor=50, maxls=50, ftol=0.00001 * _EPS),
    "uv": dict(maxiter=70000, maxfun=70000, maxcor=50, maxls=50, ftol=0.00001 * _EPS),
}


class PINN(ModelBase, PredictMixin, material.MaterialMixin):
    material_family = material.PLATE

    def __init__(self, Collo, HOLE, IC, LF, RT, UP, LW, DIST, uv_layers, dist_layers, part_layers, lb, ub,
                 partDir='', distDir='', uvDir='', *, precision="f16x3", engines=None, seed=1111, process_group=None, verbose=True,
                 always_reduce=False, collective="rccl", p2p_timeout_s=None):
        self.count = 0
        self._shift_state = {}
        self.lb = np.asarray(lb, dtype=np.float64).reshape(-1)
        self.ub = np.asarray(ub, dtype=np.float64).reshape(-1)
        self.E, self.mu, self.rho, self.hole_r = 20.0, 0.25, 1.0, 0.1          # PLATE:39-42
        self.uv_layers = [int(v) for v in uv_layers]
        self.dist_layers = [int(v) for v in dist_layers]
        self.part_layers = [int(v) for v in part_layers]
        self.verbose = verbose
        self._init_topology(process_group, always_reduce)
        if engines is None:
            engines = {k: self._default_engine(l, precision, np.asarray(Collo).shape[0])
                       for k, l in (("uv", self.uv_layers), ("dist", self.dist_layers), ("part", self.part_layers))}
        self.eng = engines
        # (net_api.NetApi's default engine; nets of other sizes find theirs in _engine_for.  The frozen 4 x 20 nets are evaluated once: their
        # path does not matter)
        self._set_engine(engines["uv"], "plate")
        self._init_rng = np.random.default_rng(seed)
        self.theta, self.adam_m, self.adam_v = {}, {}, {}
        for key, layers, d in (("dist", self.dist_layers, distDir), ("part", self.part_layers, partDir), ("uv", self.uv_layers, uvDir)):
            W, b = self.initialize_NN(layers) if d == '' else self.load_NN(d, layers)      # PLATE:96-112
            self.theta[key] = torch.from_numpy(pack_params(W, b)).to(self.device)
        self._shift_state["theta"] = self.theta["uv"]
        self.adam_m = torch.zeros_like(self.theta["uv"])
        self.adam_v = torch.zeros_like(self.theta["uv"])
        self.adam_t = 0

        def dev(a):
            return device_array(a, self.device)

        def xyt(A, shard=True):
            A = np.asarray(A, dtype=np.float64)
            s, e = self._shard(0, A.shape[0]) if shard else (0, A.shape[0])
            return A[s:e], tuple(self._device_columns(A[s:e, k] for k in range(3)))

        Collo = np.asarray(Collo, dtype=np.float64)
        self.x_c, self.y_c, self.t_c = Collo[:, 0:1], Collo[:, 1:2], Collo[:, 2:3]
        self.n_collo = Collo.shape[0]
        _, self._collo = xyt(Collo)
        HOLE = np.asarray(HOLE, dtype=np.float64)
        self.n_hole = HOLE.shape[0]
        Hs, self._hole = xyt(HOLE)
        self._hole_normals = (dev(-Hs[:, 0] / self.hole_r), dev(-Hs[:, 1] / self.hole_r))      # PLATE:457-458
        # pre-training sets: (points, targets [5 streams, 5 outs, n] or None, weight mask [5][5]); replicated, they are small
        self._dist_sets, self._part_sets = [], []
        DIST = np.asarray(DIST, dtype=np.float64)
        tg = np.zeros((5, 5, DIST.shape[0]), dtype=np.float32)
        tg[0] = DIST[:, 3:8].T
        w = np.zeros((5, 5))
        w[0, :] = 1.0
        self._dist_sets.append((xyt(DIST, False)[1], dev(tg), w, DIST.shape[0]))               # PLATE:194-198
        ICa = np.asarray(IC, dtype=np.float64)
        w = np.zeros((5, 5))
        w[3, 0] = w[3, 1] = 1.0
        self._dist_sets.append((xyt(ICa, False)[1], None, w, ICa.shape[0]))                    # PLATE:199-200 (dt_D_u, dt_D_v at IC)
        w = np.zeros((5, 5))
        w[0, :] = 1.0
        w[3, 0] = w[3, 1] = 1.0
        self._part_sets.append((xyt(ICa, False)[1], None, w, ICa.shape[0]))                    # PLATE:201-207
        for A, cols, tcol in ((LF, (0, 4), None), (RT, (2, 4), 3), (LW, (1, 4), None), (UP, (3, 4), None)):   # PLATE:208-215
            A = np.asarray(A, dtype=np.float64)
            w = np.zeros((5, 5))
            w[0, list(cols)] = 1.0
            tgt = None
            if tcol is not None:
                tg = np.zeros((5, 5, A.shape[0]), dtype=np.float32)
                tg[0, 2] = A[:, tcol]                                                          # s11_RT
                tgt = dev(tg)
            self._part_sets.append((xyt(A, False)[1], tgt, w, A.shape[0]))
        self._buf = torch.zeros(self.theta["uv"].numel() + 16, dtype=torch.float32, device=self.device)
        self._init_collective(collective, p2p_timeout_s)
        self.refresh_frozen()

    def refresh_frozen(self):
        """(Re)compute the streams of the frozen distance / particular nets on the collocation and hole points."""
        x, y, t = self._collo
        if x.numel():
            D = self.eng["dist"].net_streams(self.theta["dist"], x, y, t, self.lb, self.ub, False)
            P = self.eng["part"].net_streams(self.theta["part"], x, y, t, self.lb, self.ub, False)
            self._frozen_collo = torch.stack([D, P]).contiguous()
        x, y, t = self._hole
        if x.numel():
            D0 = self.eng["dist"].net_streams(self.theta["dist"], x, y, t, self.lb, self.ub, False)[0]
            P0 = self.eng["part"].net_streams(self.theta["part"], x, y, t, self.lb, self.ub, False)[0]
            self._aux_hole = torch.cat([D0, P0, self._hole_normals[0][None], self._hole_normals[1][None]]).contiguous()

    # ---- checkpoints (PLATE:276-306) ----------------------------------------------------------------------------------
    def save_NN(self, fileDir, TYPE=''):
        key = {"UV": "uv", "DIST": "dist", "PART": "part"}.get(TYPE)
        if key is None:
            return
        layers = {"uv": self.uv_layers, "dist": self.dist_layers, "part": self.part_layers}[key]
        self._save_net(fileDir, self.theta[key], layers)

    # ---- neural_net(X, weights, biases) (PLATE:308-320; PLATE:322-356 runs all three nets through it): net_api.NetApi ------------
    def _current_theta(self):
        return self.theta["uv"]

    def _engine_for(self, layers):
        layers = [int(v) for v in layers]
        for eng in self.eng.values():
            if [int(v) for v in eng.layers] == layers:
                return eng
        return super()._engine_for(layers)

    def _net_fields(self, eng, theta, X):
        xs = self._device_columns((X[:, k] for k in range(3)), eng.device)
        return eng.net_streams(theta, xs[0], xs[1], xs[2], self.lb, self.ub, False)[0]

    # ---- graph pieces on column arrays --------------------------------------------------------------------------------
    def _streams(self, key, x, y, t):
        xs = self._device_columns((x, y, t))
        return self.eng[key].net_streams(self.theta[key], xs[0], xs[1], xs[2], self.lb, self.ub, False)

    def _composite(self, x, y, t):
        N, D, P = (self._streams(k, x, y, t) for k in ("uv", "dist", "part"))
        F = torch.empty_like(N)
        F[0] = P[0] + D[0] * N[0]
        for k in (1, 2, 3):
            F[k] = P[k] + D[k] * N[0] + D[0] * N[k]
        F[4] = P[4] + D[4] * N[0] + 2.0 * D[3] * N[3] + D[0] * N[4]
        return F

    def net_dist(self, x, y, t):                     # PLATE:322-329
        return self._cols(self._streams("dist", x, y, t)[0])

    def net_dist_dt(self, x, y, t):                  # PLATE:331-345
        return self._cols(self._streams("dist", x, y, t)[3])

    def net_part(self, x, y, t):                     # PLATE:347-356
        S = self._streams("part", x, y, t)
        return self._cols(torch.cat([S[0], S[3, 0:2]]))

    def net_uv(self, x, y, t):                       # PLATE:358-388
        return self._cols(self._composite(x, y, t)[0])

    def net_e(self, x, y, t):                        # PLATE:390-396
        F = self._composite(x, y, t)
        return self._cols(torch.stack([F[1, 0], F[2, 1], F[2, 0] + F[1, 1]]))

    def net_vel(self, x, y, t):                      # PLATE:398-402
        F = self._composite(x, y, t)
        return self._cols(F[3, 0:2])

    def net_f_sig(self, x, y, t):                    # PLATE:404-439
        F = self._composite(x, y, t)
        E, mu, rho = self.E, self.mu, self.rho
        e11, e22, e12 = F[1, 0], F[2, 1], F[2, 0] + F[1, 1]
        sp11 = E / (1 - mu * mu) * e11 + E * mu / (1 - mu * mu) * e22
        sp22 = E * mu / (1 - mu * mu) * e11 + E / (1 - mu * mu) * e22
        sp12 = E / (2 * (1 + mu)) * e12
        f_u = F[1, 2] + F[2, 4] - rho * F[4, 0]
        f_v = F[2, 3] + F[1, 4] - rho * F[4, 1]
        return self._cols(torch.stack([f_u, f_v, F[0, 2] - sp11, F[0, 3] - sp22, F[0, 4] - sp12]))

    def net_surf_var(self, x, y, t, nx, ny):         # PLATE:441-450
        u, v, s11, s22, s12 = self.net_uv(x, y, t)
        return s11 * nx + s12 * ny, s12 * nx + s22 * ny

    def net_t(self, x, y, t):                        # PLATE:452-461
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        return self.net_surf_var(x, y, t, -x / self.hole_r, -y / self.hole_r)

    # ---- residual-adaptive refinement of the collocation set (refine.py) ----------------------------------------------
    def _score_weights(self, weights):
        """10 on each of the five collocation terms -- what loss = 10 (...) puts on them without the 1/N --, unless the caller gives five"""
        return score_weights(weights, [10.0] * 5, "(f_u, f_v, f_s11, f_s22, f_s12)")

    def _frozen_at(self, xs):
        """[2, 5, 5, n]: the streams of the frozen distance and particular nets at the device columns ``xs``"""
        D = self.eng["dist"].net_streams(self.theta["dist"], xs[0], xs[1], xs[2], self.lb, self.ub, False)
        P = self.eng["part"].net_streams(self.theta["part"], xs[0], xs[1], xs[2], self.lb, self.ub, False)
        return torch.stack([D, P]).contiguous()

    def _score_device(self, xs, frozen, w, packed=False):
        kw = {"packed": True} if packed else {}
        return self.eng["uv"].plate_residual_score(self.theta["uv"], xs[0], xs[1], xs[2], self.lb, self.ub, False, frozen, w, self.E, self.mu,
                                                   self.rho, **kw)

    def residual_score(self, x, y, t, weights=None):
        """sum_i weights[i] * f_i^2 of net_f_sig's five residuals (PLATE:404-439) per point, numpy [N,1]: the D and P streams at the points,
        then one score call on the uv net that forms the composite and the residuals in the kernel.  Default ``weights``: [10] * 5."""
        w = self._score_weights(weights)
        xs = self._device_columns((x, y, t))
        if xs[0].numel() == 0:
            return np.zeros((0, 1), dtype=np.float32)
        return self._score_device(xs, self._frozen_at(xs), w).detach().cpu().numpy().reshape(-1, 1)

    def refine_collocation(self, candidates, n_replace, weights=None, *, select="top", power=1.0, c=1.0, seed=None, stream=None, box=None, exclude=()):
        """Residual-adaptive refinement that keeps the set's size (the rule of elastic_wave.DeepHPM.refine_collocation): score this rank's rows
        with the frozen streams it holds and the ``candidates`` [Nc,3] (x, y, t) with frozen streams computed once for them; the
        K = min(n_replace, Nc, rows) lowest-scoring rows give way to the K highest-scoring candidates where those score strictly higher.
        THE FROZEN STREAMS FOLLOW THE ROW: for every replaced row the three coordinate columns AND the [2,5,5] column of the frozen D / P
        streams are overwritten with the candidate's, gathered on the device -- no second evaluation of the frozen nets.  The streams of a
        point do not depend on its place in the batch (a point is one row of a tile), so refresh_frozen() afterwards gives the same bits
        (tests/test_gpu_refine_families.py holds that).  n_collo, the 1/N weights, the workspace and the shards stay; x_c, y_c, t_c follow on
        copies.  Data parallel: no collective, every rank refines its own rows: pass rank-distinct candidates.
        ``candidates`` may be an INT (that many points drawn on the device in ``box``, default (lb, ub); stream = round * world + rank unless
        given), ``exclude`` a list of discs (xc, yc, r) -- the hole --, ``select="sample"`` draws the K candidates with probability
        ~ score^power / mean + c: all as in DeepHPM.refine_collocation.  The frozen streams of device-drawn candidates come from _frozen_at
        as for host candidates and follow the row.  The result then also holds ``candidates``, the inserted points [replaced, 3].
        Returns dict(replaced, rows, candidate_indices, score_replaced_max, score_inserted_min) like DeepHPM's; ``rows`` are row numbers of
        the whole set.  Synchronises once."""
        C = Candidates(self, candidates, 3, "(x, y, t)", select, power, c, seed, stream, box, exclude)
        w = self._score_weights(weights)
        s0, e0 = self._shard(0, self.n_collo)
        K = min(int(n_replace), C.n, e0 - s0)
        out = empty_result()
        if not C.plain:
            out["candidates"] = np.zeros((0, 3))
        if K <= 0:
            return out
        cand = C.columns(self.eng["uv"], self.device)
        frozen_cand = self._frozen_at(cand)
        s_rows = self._score_device(self._collo, self._frozen_collo, w)
        s_cand = self._score_device(cand, frozen_cand, w, packed=True)
        ri, ci, rs, cs = select_pairs(self.eng["uv"], s_rows, s_cand, K, C.keys(self.eng["uv"], s_cand, cand))
        m = int(ri.numel())
        if m == 0:
            return out
        for k in range(3):
            self._collo[k][ri] = cand[k][ci]
        self._frozen_collo[..., ri] = frozen_cand[..., ci]
        r_host, c_host = ri.cpu().numpy() + s0, ci.cpu().numpy()
        pts = C.inserted(cand, ci, c_host)
        update_host_columns(self, ("x_c", "y_c", "t_c"), r_host, np.arange(m), pts)
        out.update(replaced=m, rows=r_host, candidate_indices=c_host, score_replaced_max=float(rs.max()), score_inserted_min=float(cs.min()))
        if not C.plain:
            out["candidates"] = pts
        return out

    # ---- identification of E, mu, rho: the moment sums of the collocation residuals (material.py) ----------------------
    def _material_weights(self, n_blk):
        """what _loss_and_grad puts on the five collocation terms: 10 / n_collo each (the set is never split into blocks)"""
        return [10.0 / n_blk] * 5

    def _material_rows(self):
        return self.n_collo

    def _material_engine_sums(self, lo, hi, **kw):
        if (lo, hi) != (0, self.n_collo):
            raise ValueError("the plate trains on its whole collocation set: material sums are taken over all of it")
        x, y, t = self._collo
        if x.numel() == 0:
            return None
        return self.eng["uv"].plate_material_sums(self.theta["uv"], x, y, t, self.lb, self.ub, False, self._frozen_collo, self.E, self.mu,
                                                  self.rho, **kw)

    def callback(self, loss):
        self.count = self.count + 1
        if self.verbose and self.rank == 0:
            print('{} th iterations, Loss: {}'.format(self.count, loss))

    callback_dist = callback
    callback_part = callback

    # ---- main stage: loss = 10 (loss_f_uv + loss_f_s + loss_HOLE) wrt the uv net (PLATE:187-193,217) -----------------------
    def _loss_and_grad(self, adam=None):
        """self._buf = [grad | 8 collocation sums | 8 hole sums], all-reduced.  ``adam = (learning_rate, step)``: where the whole evaluation is one
        library call (engine.plate_step) and no collective stands in between, the Adam update rides in its reduction: returns True then."""
        P = self.theta["uv"].numel()
        buf, eng = self._buf, self.eng["uv"]
        grad = buf[:P]
        x, y, t = self._collo
        hx, hy, ht = self._hole
        if x.numel() and hx.numel() and hasattr(eng, "plate_step"):
            fold = adam is not None and not self._reduce
            eng.plate_step(self.theta["uv"], x, y, t, self.lb, self.ub, False, self._frozen_collo, [10.0 / self.n_collo] * 5,
                           (hx, hy, ht, self._aux_hole, [10.0 / self.n_hole] * 2), grad, buf[P:P + 8], buf[P + 8:P + 16], self.E, self.mu, self.rho,
                           adam=(self.adam_m, self.adam_v, adam[0], adam[1]) if fold else None)
            if self._reduce:
                all_reduce_sum(buf, self.pg, getattr(self, "collective_events", None), getattr(self, "_p2p", None))
            return fold
        buf[P:].zero_()
        wrote = False
        if x.numel():
            tw = [10.0 / self.n_collo] * 5
            eng.plate_loss_grad(self.theta["uv"], x, y, t, self.lb, self.ub, False, self._frozen_collo, tw, self.E, self.mu, self.rho,
                                grad_out=grad, accumulate=False, loss_out=buf[P:P + 8])
            wrote = True
        x, y, t = self._hole
        if x.numel():
            w = [10.0 / self.n_hole] * 2
            eng.traction_loss_grad(self.theta["uv"], x, y, t, self.lb, self.ub, False, self._aux_hole, w,
                                   grad_out=grad, accumulate=wrote, loss_out=buf[P + 8:P + 16], packed=wrote)
            wrote = True
        if not wrote:
            grad.zero_()
        if self._reduce:
            all_reduce_sum(buf, self.pg, getattr(self, "collective_events", None), getattr(self, "_p2p", None))

    def _terms(self, sums):
        out = {"loss_f_uv": float(sums[0:2].sum() / self.n_collo), "loss_f_s": float(sums[2:5].sum() / self.n_collo),
               "loss_HOLE": float(sums[8:10].sum() / self.n_hole)}
        out["loss"] = 10.0 * (out["loss_f_uv"] + out["loss_f_s"] + out["loss_HOLE"])
        return out

    def train(self, iter, learning_rate, refine=None, validate=None, identify=None):
        """Adam loop of PLATE:475-506 (whole collocation set every step).  Returns (loss_f_uv, loss_f_s, loss_HOLE, loss) lists;
        as in elastic_wave.DeepHPM.train the recorded values are those the step's gradient was taken at.  ``refine``: None, or
        dict(every, candidates, n_replace, ...): refine_collocation with device-drawn candidates behind every ``every``-th step of this call.
        ``validate``: None, or dict(every, points=(x, y, t), ref={name: column}, fields=(...)): the relative L2 of predict's fields against ``ref``
        behind every ``every``-th step, downloaded at the loop's host synchronisation into ``self.val_rec`` as (step, dict).
        ``identify``: None, or dict(params=("E", "mu"), lr=1e-3, every=1, bounds=...) as in elastic_wave.DeepHPM.train: behind every
        ``every``-th step one forward-only call takes the 12 fp64 sums of the collocation set (pinn_plate2d_material_sums, with the frozen
        streams the step uses) at the step's weights and constants, a float64 Adam on the host moves the named constants -- plane stress --,
        (step, E, mu, rho) is appended to ``self.material_rec``.  Cost, MI355X, 8x64, f16x3, 500 000 points: 1.57 ms per step with None, 2.35 with
        every=1, 1.78 with every=4 (profiles/material_family_calls.txt).  With None the loop makes exactly
        the calls it makes without the keyword.  The train_bfgs* stages leave the constants alone."""
        P = self.theta["uv"].numel()
        sched, vsched, msched = schedule(self, refine), validate_schedule(self, validate), material.schedule(self, identify)
        rec = torch.empty((iter, 16), dtype=torch.float32, device=self.device)

        def probe():
            self._loss_and_grad()
            return self._buf

        if iter > 0:
            self._settle_adjoint_shift(self.eng["uv"], probe, P)      # (E = 20 makes the plate's early residuals large)
        for it in range(iter):
            self.adam_t += 1
            if msched is not None:
                msched.before_step(it + 1, 0, self.n_collo)
            updated = self._loss_and_grad(adam=(learning_rate, self.adam_t))
            rec[it].copy_(self._buf[P:])
            if not updated:
                self.eng["uv"].adam_step(self.theta["uv"], self.adam_m, self.adam_v, self._buf[:P], learning_rate, self.adam_t)
            if self.verbose and it % 10 == 0 and self.rank == 0:
                print('It: %d, Loss: %.6e' % (it, self._terms(rec[it].detach().cpu().numpy())["loss"]))
            if msched is not None:
                msched.after_step()
            if sched is not None:
                sched.after_step(it + 1)
            if vsched is not None:
                vsched.after_step(it + 1)
        sums = rec.detach().cpu().numpy()
        if vsched is not None:
            vsched.flush()
        self._check_collective()                     # (behind the loop's one host synchronisation)
        tms = [self._terms(s) for s in sums]
        return ([t["loss_f_uv"] for t in tms], [t["loss_f_s"] for t in tms], [t["loss_HOLE"] for t in tms], [t["loss"] for t in tms])

    def _bfgs(self, key, fun, options):
        import scipy.optimize
        x0 = self.theta[key].detach().cpu().numpy().astype(np.float64)
        res = scipy.optimize.minimize(fun, x0, jac=True, method='L-BFGS-B', options=options)
        self.theta[key].copy_(torch.from_numpy(res.x.astype(np.float32)).to(self.device))
        return res

    def train_bfgs(self, options: Optional[dict] = None, backend: str = "scipy"):          # PLATE:508-526
        """backend="torch": the optimizer runs on the device too (optim.lbfgs_on_device); backend="hip": the library's own L-BFGS, no host
        round trip per evaluation (optim.lbfgs_hip: the callbacks arrive in batches).  Any other name raises ValueError."""
        check_backend(backend)

        def evaluate():
            self._loss_and_grad()
            return self._buf

        c = np.zeros(16)                                 # _terms(...)["loss"] as coefficients of the 16 sums
        c[0:5], c[8:10] = 10.0 / self.n_collo, 10.0 / self.n_hole
        return self._lbfgs_stage(backend, self.eng["uv"], self.theta["uv"], evaluate, lambda sums: self._terms(sums)["loss"], c.tolist(),
                                 dict(BFGS_OPTIONS["uv"], **(options or {})))

    def _pretrain_loss_grad(self, key, sets):
        """sum over sets of mean-square terms (PLATE:194-215); returns (loss, grad) on the host."""
        eng, th = self.eng[key], self.theta[key]
        if hasattr(eng, "stream_loss_grad_multi"):
            # one library call for all sets (4 x 20 nets: repack | one persistent launch | one reduction) and one copy to the host:
            # buf = [grad | 8 sums per set], the sums normalised by the call's largest weight
            P, m = th.numel(), len(sets)
            buf = self.__dict__.setdefault("_pre_buf", {}).get(key)
            if buf is None or buf.numel() != P + 8 * m:
                buf = self._pre_buf[key] = torch.zeros(P + 8 * m, dtype=torch.float32, device=self.device)
            rows = [(x, y, t, tg, (w / n).tolist(), buf[P + 8 * k:P + 8 * k + 8]) for k, ((x, y, t), tg, w, n) in enumerate(sets)]
            eng.stream_loss_grad_multi(th, rows, self.lb, self.ub, False, grad_out=buf[:P], accumulate=False)
            host = buf.detach().cpu().numpy().astype(np.float64)
            wmax = max(float(np.abs(w).max() / n) for _, _, w, n in sets)
            nout = int(eng.layers[-1])
            total = sum(host[P + 8 * k:P + 8 * k + nout].sum() for k in range(m))
            return float(np.float32(wmax) * total), host[:P].copy()
        grad = torch.zeros_like(th)
        total = torch.zeros((), dtype=torch.float32, device=self.device)
        for (x, y, t), tg, w, n in sets:
            wl = (w / n).tolist()
            ls, _ = eng.stream_loss_grad(th, x, y, t, self.lb, self.ub, False, tg, wl, grad_out=grad, accumulate=True)
            total = total + ls.sum() * float(w.max() / n)           # kernel sums are normalised by max|w|
        return float(total.item()), grad.detach().cpu().numpy().astype(np.float64)

    def _pretrain_coeffs(self, key, sets):
        """c with  loss = sum_j c[j] * buf[P + j]  for the buffer _pretrain_enqueue fills (8 sums per set): the library normalises the sums it
        reports by the largest weight -- of the whole call where all sets go in one call, of each set otherwise.  No launch."""
        eng = self.eng[key]
        nout = int(eng.layers[-1])
        c = np.zeros((len(sets), 8))
        per_set = [float(np.abs(w).max() / n) for _, _, w, n in sets]
        for k in range(len(sets)):
            c[k, :nout] = max(per_set) if hasattr(eng, "stream_loss_grad_multi") else per_set[k]
        return c.reshape(-1)

    def _pretrain_enqueue(self, key, sets):
        """The pre-training loss and gradient left on the device in buf = [grad | 8 sums per set] (loss = _pretrain_coeffs . sums); nothing
        synchronises.  One library call for all sets where the engine has it."""
        eng, th = self.eng[key], self.theta[key]
        P, m = th.numel(), len(sets)
        buf = self.__dict__.setdefault("_pre_buf", {}).get(key)
        if buf is None or buf.numel() != P + 8 * m:
            buf = self._pre_buf[key] = torch.zeros(P + 8 * m, dtype=torch.float32, device=self.device)
        if hasattr(eng, "stream_loss_grad_multi"):
            rows = [(x, y, t, tg, (w / n).tolist(), buf[P + 8 * k:P + 8 * k + 8]) for k, ((x, y, t), tg, w, n) in enumerate(sets)]
            eng.stream_loss_grad_multi(th, rows, self.lb, self.ub, False, grad_out=buf[:P], accumulate=False)
        else:
            for k, ((x, y, t), tg, w, n) in enumerate(sets):
                eng.stream_loss_grad(th, x, y, t, self.lb, self.ub, False, tg, (w / n).tolist(), grad_out=buf[:P], accumulate=k > 0,
                                     loss_out=buf[P + 8 * k:P + 8 * k + 8])
        return buf

    def _pretrain(self, key, sets, cb, options, backend="scipy"):
        check_backend(backend)
        if backend != "scipy":
            eng, th = self.eng[key], self.theta[key]
            P = th.numel()
            opts = dict(BFGS_OPTIONS[key], **(options or {}))
            c = self._pretrain_coeffs(key, sets)

            def evaluate():
                return self._pretrain_enqueue(key, sets)

            if backend == "hip":
                # ScipyOptimizerInterface(1000 * loss_X, ...) PLATE:220,230: the factor goes into the coefficients and the gradient scale;
                # the callbacks see the unscaled loss (PLATE:527-559).  The stream losses have no adjoint-shift retry: no ladder.
                res = lbfgs_hip(eng, th, evaluate, P, (1000.0 * c).tolist(), opts, cb, grad_scale=1000.0, loss_scale=1000.0,
                                check=self._check_collective, ladder=False, what=f"pre-training of the {key!r} net")
            else:
                def loss_and_grad():
                    buf = evaluate()
                    loss = float(c @ buf[P:].detach().cpu().numpy().astype(np.float64))
                    if not (np.isfinite(loss) and bool(torch.isfinite(buf[:P]).all())):
                        raise FloatingPointError(f"pre-training of the {key!r} net produced a non-finite loss or gradient "
                                                 f"(loss = {loss}); restart from other weights or use precision='bf16x3'")
                    return 1000.0 * loss, 1000.0 * buf[:P]
                res = lbfgs_on_device(th, loss_and_grad, opts, lambda f: cb(f / 1000.0))
            self.refresh_frozen()
            return res

        def fun(th):
            self.theta[key].copy_(torch.from_numpy(th.astype(np.float32)).to(self.device))
            loss, g = self._pretrain_loss_grad(key, sets)
            if not (np.isfinite(loss) and np.isfinite(g).all()):
                # the stream losses have no adjoint-shift retry (pinn_stream_loss_grad evaluates small nets on O(1) targets); a
                # non-finite value here means the optimizer was handed a wild point -- say so instead of feeding NaN to scipy
                raise FloatingPointError(f"pre-training of the {key!r} net produced a non-finite loss or gradient "
                                         f"(loss = {loss}); restart from other weights or use precision='bf16x3'")
            cb(loss)                                                 # fetches = [loss_DIST] / [loss_PART]: the callbacks see the unscaled loss (PLATE:527-559)
            return 1000.0 * loss, 1000.0 * g                         # ScipyOptimizerInterface(1000 * loss_X, ...) PLATE:220,230
        res = self._bfgs(key, fun, dict(BFGS_OPTIONS[key], **(options or {})))
        self.refresh_frozen()
        return res

    def train_bfgs_dist(self, options: Optional[dict] = None, backend: str = "scipy"):     # PLATE:527-544
        """backend: "scipy" (default), "torch" or "hip" as in train_bfgs; with "hip" the gradient never leaves the device"""
        return self._pretrain("dist", self._dist_sets, self.callback_dist, options, backend)

    def train_bfgs_part(self, options: Optional[dict] = None, backend: str = "scipy"):     # PLATE:546-559
        return self._pretrain("part", self._part_sets, self.callback_part, options, backend)

    # ---- inference / diagnostics ----------------------------------------------------------------------------------------
    def predict(self, x_star, y_star, t_star):       # PLATE:561-570
        F = self._composite(x_star, y_star, t_star)
        return self._cols(torch.stack([F[0, 0], F[0, 1], F[0, 2], F[0, 3], F[0, 4], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]]))

    # predict on the device (validate.PredictMixin): D and P from net_streams as _frozen_at does, the uv net through the predict head
    PREDICT_FIELDS = ("u", "v", "s11", "s22", "s12", "e11", "e22", "e12")
    PREDICT_INPUTS = ("x", "y", "t")
    VALIDATE_FIELDS = ("u", "v", "s11", "s22", "s12")

    def _predict_engine(self):
        return self.eng["uv"]

    def _predict_aux(self, xs):
        """the frozen D / P streams at the points: they do not change while the uv net trains, so train(validate=...) evaluates them once"""
        return self._frozen_at(xs) if xs[0].numel() else None

    def _predict_cols(self, xs, frozen=None):
        if xs[0].numel() == 0:
            return torch.empty((8, 0), dtype=torch.float32, device=self.device)
        return self.eng["uv"].plate_predict(self.theta["uv"], xs[0], xs[1], xs[2], self.lb, self.ub, False,
                                            self._frozen_at(xs) if frozen is None else frozen)

    def predict_D(self, x_star, y_star, t_star):     # PLATE:572-578
        return self.net_dist(x_star, y_star, t_star)

    def predict_P(self, x_star, y_star, t_star):     # PLATE:580-586
        return self._cols(self._streams("part", x_star, y_star, t_star)[0])

    def getloss(self):                               # PLATE:588-612
        P = self.theta["uv"].numel()
        self._loss_and_grad()
        tm = self._terms(self._buf[P:].detach().cpu().numpy())
        self._check_collective()
        tm["loss_PART"] = self._pretrain_loss_grad("part", self._part_sets)[0]
        tm["loss_DIST"] = self._pretrain_loss_grad("dist", self._dist_sets)[0]
        if self.verbose and self.rank == 0:
            for k in ("loss_f_uv", "loss_f_s", "loss_HOLE", "loss", "loss_PART", "loss_DIST"):
                print(k, tm[k])
        return tm
