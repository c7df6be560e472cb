"""Identification of the material constants (E, mu, rho) while the net trains: the wave, plate and 3-D families.

The seven residuals of net_f_sig (INF:221-265) are linear in the Hooke coefficients (c1, c2, G) and in rho, so the derivative of a collocation
loss L = sum_i w_i sum_n f_i(n)^2 by each of the four is a moment sum of streams the forward pass already carries -- the 14 doubles of
pinn_wave2d_material_sums (include/pinn_hip.h), M_k below:

    dL/dc1 = -2 (w4 M7 + w5 M10)     dL/dc2 = -2 (w4 M8 + w5 M9)     dL/dG = -2 w6 M11     dL/drho = -2 (w0 M12 + w1 M13)

No reverse pass is involved; what is left to the host is the chain rule from (c1, c2, G) to (E, mu) in either plane mode (``hooke_jacobian``),
a float64 Adam on three numbers (``HostAdam``: the TF1 rule of pinn_adam_step) and the bookkeeping of ``train(identify=...)``
(``MaterialSchedule``).

The plate's five residuals (PLATE:404-439, plane stress) and the twelve of the 3-D family (stated term by term in include/pinn_hip.h) are linear in the same four
numbers; a ``Family`` says how many sums and weights a family has and which sums and weights make d/dc1, d/dc2, d/dG and d/drho.  The 3-D
coefficients (lambda + 2G, lambda, G) ARE the plane-strain ``hooke()``: there is no third formula.
"""
from __future__ import annotations

import math

from collections import namedtuple

import numpy as np
import torch

from .refine import score_weights

NAMES = ("E", "mu", "rho")
N_SUMS = 14
DEFAULT_BOUNDS = {"mu": (0.0, 0.49)}

# n_sums, n_weights: the lengths of a family's sums and of its loss weights (one per residual, the first n_weights sums are the squares);
# c1, c2, G, rho: ((weight index, sum index), ...) -- dL/dc = -2 sum_j w[weight_j] M[sum_j];  plane_strain: the hooke() mode of the family;
# residuals: the names of the weights, for messages
Family = namedtuple("Family", "name n_sums n_weights c1 c2 G rho plane_strain residuals")
WAVE = Family("wave", 14, 7, ((4, 7), (5, 10)), ((4, 8), (5, 9)), ((6, 11),), ((0, 12), (1, 13)), True,
              "(f_u, f_v, f_ut, f_vt, f_s11, f_s22, f_s12)")
WAVE_PLANE_STRESS = WAVE._replace(plane_strain=False)
PLATE = Family("plate", 12, 5, ((2, 5), (3, 8)), ((2, 6), (3, 7)), ((4, 9),), ((0, 10), (1, 11)), False,
               "(f_u, f_v, f_s11, f_s22, f_s12)")
# (c1, c2, G) = (lambda + 2G, lambda, G): the plane-strain hooke()
NC3D = Family("nc3d", 24, 12, ((6, 12), (7, 14), (8, 16)), ((6, 13), (7, 15), (8, 17)), ((9, 18), (10, 19), (11, 20)),
              ((0, 21), (1, 22), (2, 23)), True, "(f_u, f_v, f_w, f_ut, f_vt, f_wt, f_s11, f_s22, f_s33, f_s12, f_s13, f_s23)")
MAX_SUMS = NC3D.n_sums


def family_of(family):
    """``family`` as a Family: one is returned as it is; True / False (the argument ``plane_strain`` of the wave family) mean the wave's"""
    if isinstance(family, Family):
        return family
    return WAVE if family else WAVE_PLANE_STRESS


def hooke(E, mu, plane_strain=True):
    """(c1, c2, G): sp11 = c1 e11 + c2 e22, sp22 = c2 e11 + c1 e22, sp12 = G e12 -- plane strain INF:238-241, plane stress PLATE:416-418"""
    if plane_strain:
        coef = E / ((1.0 + mu) * (1.0 - 2.0 * mu))
        c1, c2 = coef * (1.0 - mu), coef * mu
    else:
        c1, c2 = E / (1.0 - mu * mu), E * mu / (1.0 - mu * mu)
    return c1, c2, E / (2.0 * (1.0 + mu))


def hooke_jacobian(E, mu, plane_strain=True):
    """d(c1, c2, G) / d(E, mu) as a [3, 2] array (rows c1, c2, G; columns E, mu).  All three coefficients are proportional to E."""
    c1, c2, G = hooke(E, mu, plane_strain)
    if plane_strain:
        D = (1.0 + mu) * (1.0 - 2.0 * mu)
        coef, dcoef = E / D, E * (1.0 + 4.0 * mu) / (D * D)
        dc1, dc2 = dcoef * (1.0 - mu) - coef, dcoef * mu + coef
    else:
        q = 1.0 - mu * mu
        dc1, dc2 = 2.0 * E * mu / (q * q), E * (1.0 + mu * mu) / (q * q)
    dG = -E / (2.0 * (1.0 + mu) ** 2)
    return np.array([[c1 / E, dc1], [c2 / E, dc2], [G / E, dG]], dtype=np.float64)


def gradient(sums, weights, E, mu, rho, family=True):
    """dict(E, mu, rho) -> dL/dE, dL/dmu, dL/drho of L = sum_i weights[i] * sums[i] (i < the family's n_weights) at the constants the ``sums``
    were taken at.  ``family``: a Family (WAVE, PLATE, NC3D), or the wave family's ``plane_strain`` flag."""
    fam = family_of(family)
    M = np.asarray(sums, dtype=np.float64).reshape(-1)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if M.size != fam.n_sums or w.size != fam.n_weights:
        raise ValueError(f"gradient: {fam.n_sums} sums and {fam.n_weights} weights {fam.residuals}")

    def moment(pairs):
        return -2.0 * sum(w[i] * M[k] for i, k in pairs)
    d_c = np.array([moment(fam.c1), moment(fam.c2), moment(fam.G)])
    d_E, d_mu = d_c @ hooke_jacobian(float(E), float(mu), fam.plane_strain)
    return {"E": float(d_E), "mu": float(d_mu), "rho": float(moment(fam.rho))}


class HostAdam:
    """The TF1 Adam rule of pinn_adam_step in float64 on a few host numbers: epsilon added to the uncorrected sqrt(v), the bias correction folded
    into the step size"""

    def __init__(self, n, beta1=0.9, beta2=0.999, eps=1e-8):
        self.m, self.v, self.t = np.zeros(n), np.zeros(n), 0
        self.beta1, self.beta2, self.eps = beta1, beta2, eps

    def step(self, x, g, lr):
        self.t += 1
        g = np.asarray(g, dtype=np.float64)
        self.m = self.beta1 * self.m + (1.0 - self.beta1) * g
        self.v = self.beta2 * self.v + (1.0 - self.beta2) * g * g
        lr_t = lr * math.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        return np.asarray(x, dtype=np.float64) - lr_t * self.m / (np.sqrt(self.v) + self.eps)


class MaterialSchedule:
    """train(..., identify=dict(params=("E", "mu"), lr=1e-3, every=1, bounds=dict(mu=(0.0, 0.49)))): behind every ``every``-th step of the call
    the named constants take one Adam step along the derivative of the step's collocation loss.  ``before_step(j, lo, hi, packed)`` (j = 1, 2,
    ... counted over the whole train call) enqueues the sums on the step's block BEFORE the step call -- at the weights and constants the step's
    gradient is taken at -- and sends them towards the host (model._material_sums_async); ``after_step()``, called once the step is enqueued,
    waits for that copy alone, updates the constants on the model and appends (j, E, mu, rho) to ``model.material_rec``: the next step's call
    sees the new values.  E and rho are optimised as logarithms (they stay positive), mu directly, clipped to its bounds.  The optimiser state is
    one per model (``model._material_adam``) and survives between train calls that name the same parameters.  Data parallel: the sums are
    all-reduced, every rank makes the same update."""

    def __init__(self, model, identify):
        kw = dict(identify)
        self.params = tuple(kw.pop("params", ("E", "mu")))
        self.lr, self.every = float(kw.pop("lr", 1e-3)), int(kw.pop("every", 1))
        self.bounds = dict(DEFAULT_BOUNDS, **kw.pop("bounds", {}))
        if kw:
            raise ValueError(f"identify: unknown entries {sorted(kw)}")
        if not self.params or any(p not in NAMES for p in self.params) or len(set(self.params)) != len(self.params):
            raise ValueError(f"identify: params is a non-empty subset of {NAMES}")
        if any(p not in NAMES for p in self.bounds):
            raise ValueError(f"identify: bounds are given for {NAMES}")
        if self.every < 1 or not self.lr > 0.0:
            raise ValueError("identify: every >= 1 and lr > 0")
        self.model = model
        self.pending = None
        state = getattr(model, "_material_adam", None)
        if state is None or state[0] != self.params:
            model._material_adam = (self.params, HostAdam(len(self.params)))
        self.adam = model._material_adam[1]
        if not hasattr(model, "material_rec"):
            model.material_rec = []

    def before_step(self, step, lo, hi, packed=False):
        if step % self.every == 0:
            self.pending = (step, hi - lo, self.model._material_sums_async(lo, hi, packed))

    def after_step(self):
        if self.pending is None:
            return
        step, n_blk, fetch = self.pending
        self.pending = None
        m = self.model
        g = gradient(fetch(), m._material_weights(n_blk), m.E, m.mu, m.rho, getattr(m, "material_family", WAVE))
        cur = {"E": float(m.E), "mu": float(m.mu), "rho": float(m.rho)}
        # optimisation variables: log E, mu, log rho  (d/dlog x = x d/dx)
        x = [cur[p] if p == "mu" else math.log(cur[p]) for p in self.params]
        gx = [g[p] if p == "mu" else cur[p] * g[p] for p in self.params]
        for p, v in zip(self.params, self.adam.step(x, gx, self.lr)):
            v = float(v) if p == "mu" else math.exp(float(v))
            if p in self.bounds:
                v = min(max(v, float(self.bounds[p][0])), float(self.bounds[p][1]))
            cur[p] = v
        m.E, m.mu, m.rho = cur["E"], cur["mu"], cur["rho"]
        m.material_rec.append((step, m.E, m.mu, m.rho))


def schedule(model, identify):
    """the MaterialSchedule of train(identify=...), or None for identify=None"""
    return None if identify is None else MaterialSchedule(model, identify)


def pinned_sums():
    """the pinned host buffer and the event sums_to_host works with (one pair per model: a fetch precedes the next send)"""
    return torch.empty(MAX_SUMS, dtype=torch.float64, pin_memory=True), torch.cuda.Event()


def sums_to_host(sums: torch.Tensor, pinned=None):
    """Send the device tensor ``sums`` (float64, a family's n_sums) towards the host and return fetch() -> numpy of that length.  On a GPU: a copy into the pinned buffer
    of ``pinned`` (pinned_sums()) and its event recorded behind the copy on the current stream -- fetch() waits for that event alone, so work
    enqueued after this call does not delay it.  A host tensor is returned as it is."""
    if not sums.is_cuda:
        return lambda: sums.detach().numpy().astype(np.float64)
    host, ev = pinned if pinned is not None else pinned_sums()
    host = host[:sums.numel()]
    host.copy_(sums, non_blocking=True)
    ev.record(torch.cuda.current_stream(sums.device))

    def fetch():
        ev.synchronize()
        return host.numpy().copy()
    return fetch


class MaterialMixin:
    """material_sums, material_gradient and the hooks MaterialSchedule calls, for a model class with sharded collocation rows.  The class
    names its ``material_family`` and gives ``_material_weights(n_blk)`` (what its training step puts on the collocation terms of a block of
    n_blk points), ``_material_rows()`` (the rows of the whole collocation set) and ``_material_engine_sums(lo, hi, **kw)``: the engine's
    sums call over this rank's part of the rows [lo, hi) as a float64 device tensor, or None where the rank holds none of them."""
    material_family = WAVE

    def _material_sums_device(self, lo, hi, packed=False):
        """the family's sums over the rows [lo, hi) of the collocation set as a float64 tensor on the engine's device: this rank's rows, then
        summed over the process group by torch.distributed.all_reduce (whatever ``collective`` is: the P2P kernel is for the gradient
        buffer).  No host synchronisation."""
        sums = self._material_engine_sums(lo, hi, **({"packed": True} if packed else {}))
        if sums is None:
            sums = torch.zeros(self.material_family.n_sums, dtype=torch.float64, device=self.device)
        if self._reduce:
            torch.distributed.all_reduce(sums, group=self.pg)
        return sums

    def _material_sums_async(self, lo, hi, packed=False):
        """_material_sums_device on its way to the host: returns fetch() -> numpy, which waits for nothing enqueued after this call"""
        if self.device.type == "cuda" and not hasattr(self, "_material_pinned"):
            self._material_pinned = pinned_sums()
        return sums_to_host(self._material_sums_device(lo, hi, packed), getattr(self, "_material_pinned", None))

    def material_sums(self, idx_start=0, idx_end=None):
        """The family's sums (include/pinn_hip.h: pinn_wave2d_material_sums, pinn_plate2d_material_sums, pinn_nc3d_material_sums) over the
        rows [idx_start, idx_end) of the collocation set -- default: the whole set -- at the current weights and constants, host numpy: the
        sums of squared residuals of net_f_sig, then the moment sums.  Data parallel: every rank computes its shard's rows and gets the
        total."""
        hi = self._material_rows() if idx_end is None else int(idx_end)
        out = self._material_sums_async(int(idx_start), hi)()
        self._check_collective()
        return out

    def material_gradient(self, weights=None):
        """dict(E, mu, rho) -> the derivative of the collocation loss over the whole set by each constant (gradient of material_sums()).
        Default ``weights``: the case's layout over n, as the training step folds them."""
        fam = self.material_family
        w = score_weights(weights, self._material_weights(self._material_rows()), fam.residuals)
        return gradient(self.material_sums(), w, self.E, self.mu, self.rho, fam)
