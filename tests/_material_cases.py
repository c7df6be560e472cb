"""Cases and references shared by the material-identification tests (test_emulated_material.py, test_gpu_material.py, test_material_host.py): the
float64 reference of the 14 sums of pinn_wave2d_material_sums from a fields array, the bound of the head's own rounding, the float64 oracle's
sums and a CPU stand-in engine that serves them.  Everything here is computed on the host; the cached references are never written to."""
import functools

import numpy as np
import torch

from oracle import pinn_oracle as po
from tests import _refine_cases as RC
from tests._oracle_engine import OracleEngine

fresh_net, points, collocation_set, trained_net = RC.fresh_net, RC.points, RC.collocation_set, RC.trained_net
PRIMARY_LINES, PRIMARY_N, LB, UB, EPS32 = RC.PRIMARY_LINES, RC.PRIMARY_N, RC.LB, RC.UB, RC.EPS32
SECONDARY_NETS, SECONDARY_N = RC.SECONDARY_NETS, RC.SECONDARY_N
NSUMS = 14
CONSTS = (2.5, 0.25, 1.0, True)
CONSTS_GENERAL = ((7.3, 0.31, 1.9, True), (7.3, 0.31, 1.9, False))


def sums_from_fields(F, E=2.5, mu=0.25, rho=1.0, plane_strain=True):
    """PRIMARY reference: the 14 formulas in float64, with float64 coefficients, on the fields array F [4,7,n] (value, d/dx, d/dy, d/dt).
    Returns (sums [14], bound [14], scale [14]):
      bound_k = 8 eps32 sum_n a_i(n)^2 (k < 7),  8 eps32 sum_n a_i(n) g^(n) (k >= 7)  -- the head's rounding alone: at most 4 roundings in f_i, 1 in
      e12, 1 in the product, the fp32 rounding of c1, c2, G, and slack; a_i = the sum of the absolute values of the terms of f_i with their
      coefficients, g^ = |X0|, |Y1|, |X0|, |Y1|, |Y0| + |X1|, |T2|, |T3|;
      scale_k = bound_k / (8 eps32), what errors are normalised by (never |sum_k|: the moment sums cancel at a trained net)."""
    F = np.asarray(F, dtype=np.float64)
    V, X, Y, T = F[0], F[1], F[2], F[3]
    c1, c2, G = po.hooke_coeffs(E, mu, plane_strain)
    terms = [(X[4], Y[6], -rho * T[2]), (Y[5], X[6], -rho * T[3]), (T[0], -V[2]), (T[1], -V[3]),
             (V[4], -c1 * X[0], -c2 * Y[1]), (V[5], -c2 * X[0], -c1 * Y[1]), (V[6], -G * Y[0], -G * X[1])]
    f = [sum(tt) for tt in terms]
    a = [sum(np.abs(v) for v in tt) for tt in terms]
    e11, e22, e12 = X[0], Y[1], Y[0] + X[1]
    pairs = [(4, e11, np.abs(X[0])), (4, e22, np.abs(Y[1])), (5, e11, np.abs(X[0])), (5, e22, np.abs(Y[1])),
             (6, e12, np.abs(Y[0]) + np.abs(X[1])), (0, T[2], np.abs(T[2])), (1, T[3], np.abs(T[3]))]
    sums = [float((fi * fi).sum()) for fi in f] + [float((f[i] * g).sum()) for i, g, _ in pairs]
    scale = [float((ai * ai).sum()) for ai in a] + [float((a[i] * gh).sum()) for i, _, gh in pairs]
    scale = np.asarray(scale)
    return np.asarray(sums), 8.0 * EPS32 * scale, scale


def oracle_fields(flat, layers, X, dtype=np.float64, normalize=True):
    """the oracle's forward in `dtype` as a fields array [4,7,n]"""
    out = po.wave2d_fields(np.asarray(flat, dtype=dtype), list(layers), X[:, 0].astype(dtype), X[:, 1].astype(dtype), X[:, 2].astype(dtype), LB, UB,
                           normalize, dtype=dtype)
    return np.stack([out["Y"].T] + [d.T for d in out["dY"]])


def oracle_sums(flat, layers, X, consts=CONSTS, dtype=np.float64, normalize=True):
    """SECONDARY reference: the 14 sums from the oracle's own forward in `dtype`; float64: formulas in float64; float32: the head in numpy float32
    on the float32 fields, summed in float64 -- what the device head does.  Returns (sums, scale)."""
    F = oracle_fields(flat, layers, X, dtype, normalize)
    if dtype == np.float64:
        s, _, scale = sums_from_fields(F, *consts)
        return s, scale
    return head_float32(F, *consts), sums_from_fields(F, *consts)[2]


def head_float32(F, E=2.5, mu=0.25, rho=1.0, plane_strain=True):
    """the head in numpy float32 on a float32 fields array (coefficients rounded to float32 once), products and sums in float64"""
    F = np.asarray(F, dtype=np.float32)
    V, X, Y, T = F[0], F[1], F[2], F[3]
    c1, c2, G = (np.float32(v) for v in po.hooke_coeffs(E, mu, plane_strain))
    rho = np.float32(rho)
    e11, e22, e12 = X[0], Y[1], Y[0] + X[1]
    f = [X[4] + Y[6] - rho * T[2], Y[5] + X[6] - rho * T[3], T[0] - V[2], T[1] - V[3],
         V[4] - (c1 * e11 + c2 * e22), V[5] - (c2 * e11 + c1 * e22), V[6] - G * e12]
    d = lambda v: np.asarray(v, dtype=np.float64)
    pairs = [(4, e11), (4, e22), (5, e11), (5, e22), (6, e12), (0, T[2]), (1, T[3])]
    return np.asarray([float((d(fi) ** 2).sum()) for fi in f] + [float((d(f[i]) * d(g)).sum()) for i, g in pairs])


def scaled_error(sums, ref, scale):
    """max_k |sums_k - ref_k| / S_k"""
    return float((np.abs(np.asarray(sums, np.float64) - ref) / scale).max())


@functools.lru_cache(maxsize=None)
def secondary_case(name):
    """(layers, flat, X, float64 oracle sums, scale, metric of the float32 oracle run): the bar is 6 x the float32 oracle's own error"""
    if name == "inf20s":
        layers, flat = trained_net()
    else:
        layers = [3] + (4 * [32] if name == "xavier4x32" else 8 * [64]) + [7]
        flat = fresh_net(tuple(layers))
    X = collocation_set(SECONDARY_N)
    ref, scale = oracle_sums(flat, layers, X)
    s32, _ = oracle_sums(flat, layers, X, dtype=np.float32)
    return layers, flat, X, ref, scale, scaled_error(s32, ref, scale)


class OracleMaterialEngine(OracleEngine):
    """OracleEngine + material_sums from the float64 oracle (the CPU side of the identification tests)"""

    def for_layers(self, layers):
        return OracleMaterialEngine(layers)

    def material_sums(self, params, x, y, t, lb, ub, normalize, E=2.5, mu=0.25, rho=1.0, plane_strain=True, out=None, packed=False):
        self.calls.append(("material", x.numel()))
        o = po.wave2d_fields(self._np(params), self.layers, self._np(x), self._np(y), self._np(t), lb, ub, normalize)
        s = sums_from_fields(np.stack([o["Y"].T] + [d.T for d in o["dY"]]), E, mu, rho, plane_strain)[0] if x.numel() else np.zeros(NSUMS)
        if out is None:
            out = torch.zeros(NSUMS, dtype=torch.float64)
        out.copy_(torch.from_numpy(s))
        return out
