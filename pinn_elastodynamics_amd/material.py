"""Identification of the material constants (E, mu, rho) of the wave family while the net trains.

The seven residuals of net_f_sig (INF:221-265) are linear in the Hooke coefficients (c1, c2, G) and in rho, so the derivative of a collocation
loss L = sum_i w_i sum_n f_i(n)^2 by each of the four is a moment sum of streams the forward pass already carries -- the 14 doubles of
pinn_wave2d_material_sums (include/pinn_hip.h), M_k below:

    dL/dc1 = -2 (w4 M7 + w5 M10)     dL/dc2 = -2 (w4 M8 + w5 M9)     dL/dG = -2 w6 M11     dL/drho = -2 (w0 M12 + w1 M13)

No reverse pass is involved; what is left to the host is the chain rule from (c1, c2, G) to (E, mu) in either plane mode (``hooke_jacobian``),
a float64 Adam on three numbers (``HostAdam``: the TF1 rule of pinn_adam_step) and the bookkeeping of ``train(identify=...)``
(``MaterialSchedule``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

NAMES = ("E", "mu", "rho")
N_SUMS = 14
DEFAULT_BOUNDS = {"mu": (0.0, 0.49)}


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


def gradient(sums, weights, E, mu, rho, plane_strain=True):
    """dict(E, mu, rho) -> dL/dE, dL/dmu, dL/drho of L = sum_i weights[i] * sums[i] (i < 7) at the constants the ``sums`` were taken at"""
    M = np.asarray(sums, dtype=np.float64).reshape(-1)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if M.size != N_SUMS or w.size != 7:
        raise ValueError("gradient: 14 sums and 7 weights (f_u, f_v, f_ut, f_vt, f_s11, f_s22, f_s12)")
    d_c = np.array([-2.0 * (w[4] * M[7] + w[5] * M[10]), -2.0 * (w[4] * M[8] + w[5] * M[9]), -2.0 * w[6] * M[11]])
    d_E, d_mu = d_c @ hooke_jacobian(float(E), float(mu), plane_strain)
    return {"E": float(d_E), "mu": float(d_mu), "rho": float(-2.0 * (w[0] * M[12] + w[1] * M[13]))}


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
        g = gradient(fetch(), m._material_weights(n_blk), m.E, m.mu, m.rho, True)
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
    return torch.empty(N_SUMS, dtype=torch.float64, pin_memory=True), torch.cuda.Event()


def sums_to_host(sums: torch.Tensor, pinned=None):
    """Send the device tensor ``sums`` [14] (float64) towards the host and return fetch() -> numpy [14].  On a GPU: a copy into the pinned buffer
    of ``pinned`` (pinned_sums()) and its event recorded behind the copy on the current stream -- fetch() waits for that event alone, so work
    enqueued after this call does not delay it.  A host tensor is returned as it is."""
    if not sums.is_cuda:
        return lambda: sums.detach().numpy().astype(np.float64)
    host, ev = pinned if pinned is not None else pinned_sums()
    host.copy_(sums, non_blocking=True)
    ev.record(torch.cuda.current_stream(sums.device))

    def fetch():
        ev.synchronize()
        return host.numpy().copy()
    return fetch
