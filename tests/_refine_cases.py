"""Cases and references shared by the refinement tests (test_emulated_refine.py, test_gpu_refine.py, test_refine_host.py): the numpy reference of
pinn_select_k, its data sets, and the two references of pinn_wave2d_residual_score.  Everything here is computed on the host; the references are
built once per case (functools.lru_cache) and never written to."""
import functools
import os

import numpy as np

from oracle import pinn_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB, UB = [0.0, 0.0, 0.0], [30.0, 30.0, 20.0]
EPS32 = float(np.finfo(np.float32).eps)

# ---- selection ---------------------------------------------------------------------------------------------------------------------------------
SELECT_N = (1, 63, 64, 65, 257, 5000, 70001)
SELECT_DATA = ("random", "equal", "spikes", "top24", "ties", "special")


def select_ks(n):
    return sorted({0, 1, n // 10, n - 1, n} & set(range(0, n + 1)))


def keys_of(score):
    """the sign-flip map: a uint32 key that is monotone in the float order (-0 below +0, a positive NaN above +inf)"""
    u = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select_reference(score, k, largest):
    """order by (key descending if largest else ascending, index ascending), take k, report ascending indices"""
    key = keys_of(score).astype(np.int64)
    order = np.lexsort((np.arange(key.size), -key if largest else key))
    return np.sort(order[:k]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def select_data(kind, n):
    rng = np.random.default_rng(1000 + 7 * n + SELECT_DATA.index(kind))
    if kind == "random":                       # positive scores, as a residual measure gives
        s = rng.random(n, dtype=np.float32) ** 4 * 10.0
    elif kind == "equal":
        s = np.full(n, 0.375, dtype=np.float32)
    elif kind == "spikes":                     # zeros with a few spikes
        s = np.zeros(n, dtype=np.float32)
        m = max(1, min(5, n // 3))
        s[rng.choice(n, m, replace=False)] = rng.random(m, dtype=np.float32) + 1.0
    elif kind == "top24":                      # keys that differ in their lowest byte only: the first three radix passes decide nothing
        s = (np.uint32(0x3F000000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    elif kind == "ties":                       # few distinct values: the threshold value is held by more than k entries for every k
        s = rng.integers(0, 3, n).astype(np.float32)
    else:                                      # +-0, +inf, -inf and one NaN among signed values
        s = rng.standard_normal(n).astype(np.float32)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=np.float32)
        pos = rng.choice(n, min(n, special.size), replace=False)
        s[pos] = special[:pos.size]
    s.setflags(write=False)
    return s


# ---- score -------------------------------------------------------------------------------------------------------------------------------------
WEIGHTS = (1.0, 2.0, 3.0, 1.0, 0.5, 1.0, 2.0)                  # exact in fp32
# (name, layers, precision): one compiled line of every padded width in f16x3 (two hidden layers where the width is what is tested), the one-MFMA and
# the bf16 split mode at width 64, and the fp32 checking mode
PRIMARY_LINES = (("w32", [3] + 4 * [32] + [7], "f16x3"), ("w64", [3] + 3 * [64] + [7], "f16x3"), ("w96", [3] + 2 * [80] + [7], "f16x3"),
                 ("w128", [3] + 2 * [100] + [7], "f16x3"), ("w160", [3] + 2 * [140] + [7], "f16x3"), ("bf16", [3] + 3 * [64] + [7], "bf16"),
                 ("bf16x3", [3] + 3 * [64] + [7], "bf16x3"), ("fp32", [3] + 3 * [48] + [7], "fp32"))
PRIMARY_N = (1, 33, 2100)


@functools.lru_cache(maxsize=None)
def fresh_net(layers, seed=5):
    rng = np.random.default_rng(seed)
    Ws, bs = po.xavier_init(list(layers), rng)
    bs = [0.3 * rng.standard_normal(b.shape) for b in bs]
    flat = po.pack_params(Ws, bs)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def trained_net():
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_inf20s.npz"))
    layers = [int(v) for v in w["layers"]]
    nl = len(layers) - 1
    flat = po.pack_params([w[f"W{i}"] for i in range(nl)], [w[f"b{i}"] for i in range(nl)])
    flat.setflags(write=False)
    return layers, flat


@functools.lru_cache(maxsize=None)
def points(n, seed=1111):
    """uniform points of the reference's domain [0,30]^2 x [0,20]"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, 3)) * (np.asarray(UB) - np.asarray(LB)) + np.asarray(LB)
    X = X.astype(np.float32).astype(np.float64)        # (what the device sees)
    X.setflags(write=False)
    return X


def score_from_fields(F, w=WEIGHTS, E=2.5, mu=0.25, rho=1.0, plane_strain=True):
    """PRIMARY reference: the residual formulas (INF:221-265) in float64 on the fp32 output F [4,7,n] of pinn_wave2d_fields of the same mode.
    Returns (score [n], bound [n]); bound = 16 eps32 sum_i w_i a_i^2 with a_i the sum of the absolute values of the terms of f_i -- the rounding
    of the head alone (at most 4 roundings in f_i: relative 4 eps of a_i; the square: 2 x 4 eps + 1; the weight and the 7-term sum: 1 + 6)."""
    F = np.asarray(F, dtype=np.float64)
    V, X, Y, T = F[0], F[1], F[2], F[3]
    c1, c2, G = po.hooke_coeffs(E, mu, plane_strain)
    terms = [(X[4], Y[6], -rho * T[2]), (Y[5], X[6], -rho * T[3]), (T[0], -V[2]), (T[1], -V[3]),
             (V[4], -c1 * X[0], -c2 * Y[1]), (V[5], -c2 * X[0], -c1 * Y[1]), (V[6], -G * Y[0], -G * X[1])]
    s = np.zeros(F.shape[-1])
    b = np.zeros(F.shape[-1])
    for wi, tt in zip(w, terms):
        s += wi * sum(tt) ** 2
        b += abs(wi) * sum(np.abs(v) for v in tt) ** 2
    return s, 16.0 * EPS32 * b


def oracle_score(flat, layers, X, w=WEIGHTS, dtype=np.float64, normalize=True, E=2.5, mu=0.25, rho=1.0, plane_strain=True):
    """SECONDARY reference: the oracle's own residuals (pinn_oracle.wave2d_residuals) in `dtype`, squared and weighted in float64"""
    out = po.wave2d_fields(np.asarray(flat), list(layers), X[:, 0], X[:, 1], X[:, 2], LB, UB, normalize, dtype=dtype)
    f = po.wave2d_residuals(out["Y"], out["dY"], dtype(E), dtype(mu), dtype(rho), plane_strain).astype(np.float64)
    return (f ** 2) @ np.asarray(w, dtype=np.float64)


def rel_l2(a, ref):
    return float(np.linalg.norm(np.asarray(a, np.float64) - ref) / np.linalg.norm(ref))


SECONDARY_NETS = ("xavier4x32", "xavier8x64", "inf20s")
SECONDARY_N = 1000


@functools.lru_cache(maxsize=None)
def collocation_set(n, seed=1111):
    """The set of the secondary check: the build's collocation sampler, i.e. the box MINUS THE SOURCE DISC (INF:619-622 deletes those points, and
    refinement candidates are drawn the same way).  Inside the disc the trained net was never asked to satisfy the equations: of 1000 uniform points
    the three with the largest float64 score all lie there (s = 18, 0.66, 0.056 against a median of 6e-6), ONE of them carries 99.9 % of the L2 norm
    of s, and a relative L2 over the set degenerates into the rounding luck of that single point.  Decided from the float64 scores and the geometry
    (the uniform set had shown the degenerate metric; no device figure on this set had been seen)."""
    X = po.collocation_points(n, LB, UB, np.random.default_rng(seed))
    X = X.astype(np.float32).astype(np.float64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def secondary_case(name):
    """(layers, flat, X, float64 score, metrics of the float32 oracle run): the bar is 6 x the float32 oracle's own error, per metric"""
    if name == "inf20s":
        layers, flat = trained_net()
    else:
        layers = [3] + (4 * [32] if name == "xavier4x32" else 8 * [64]) + [7]
        flat = fresh_net(tuple(layers))
    X = collocation_set(SECONDARY_N)
    ref = oracle_score(flat, layers, X)
    s32 = oracle_score(flat.astype(np.float32), layers, X.astype(np.float32), dtype=np.float32)
    base = (rel_l2(s32, ref), rel_l2(np.sqrt(s32), np.sqrt(ref)))
    return layers, flat, X, ref, base


def refine_rule(row_score, cand_score, n_replace):
    """Section 4 of the issue in numpy on given scores: K lowest rows against K highest candidates (ties to the lowest index), candidates by score
    descending, rows ascending, replace where strictly larger.  Returns (rows, candidates) in pairing order."""
    K = min(n_replace, cand_score.size, row_score.size)
    ci = select_reference(cand_score, K, True)
    ri = select_reference(row_score, K, False)
    ci = ci[np.argsort(-keys_of(cand_score[ci]).astype(np.int64), kind="stable")]          # (key order: a NaN ranks above +inf on both sides)
    ri = ri[np.argsort(keys_of(row_score[ri]).astype(np.int64), kind="stable")]
    keep = cand_score[ci] > row_score[ri]
    return ri[keep].astype(np.int64), ci[keep].astype(np.int64)
