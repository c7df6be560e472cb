"""Cases and references shared by the refinement tests of the plate and 3-D families (test_emulated_refine_families.py,
test_gpu_refine_families.py, test_refine_families_host.py): the two references of pinn_plate2d_residual_score / pinn_nc3d_residual_score.
Everything here is computed on the host; the references are built once per case (functools.lru_cache) and never written to.  What is family-
agnostic (refine_rule, select_reference, rel_l2, EPS32, points) comes from tests/_refine_cases.py."""
import functools
import os

import numpy as np

from oracle import golden_points as gp
from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests._refine_cases import EPS32, rel_l2  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLATE_LB, PLATE_UB = [0.0, 0.0, 0.0], [0.5, 0.5, 10.0]                       # the quarter plate (PLATE:881-882); the class never normalises
NC3D_LB, NC3D_UB = [0.0, 0.0, -30.0, 0.0], [30.0, 30.0, 0.0, 15.0]           # the half space of BASELINE configs[4]
HEAD_C = 24.0          # rounding count of the score heads, see plate_score_from_streams / nc3d_score_from_fields

# weights distinct, exact in fp32, one zero
PLATE_WEIGHTS = (1.0, 2.0, 0.0, 0.5, 3.0)
NC3D_WEIGHTS = (1.0, 2.0, 3.0, 0.5, 0.0, 1.5, 0.25, 4.0, 0.75, 2.5, 1.25, 0.125)

# (name, hidden layers, precision): one compiled line of every padded width in f16x3, the bf16 split mode at width 64, the fp32 checking mode
_LINES = (("w32", 4 * [32], "f16x3"), ("w64", 3 * [64], "f16x3"), ("w96", 2 * [80], "f16x3"), ("w128", 2 * [100], "f16x3"),
          ("w160", 2 * [140], "f16x3"), ("bf16x3", 3 * [64], "bf16x3"), ("fp32", 3 * [48], "fp32"))
PLATE_LINES = tuple((nm, [3] + h + [5], p) for nm, h, p in _LINES)
NC3D_LINES = tuple((nm, [4] + h + [12], p) for nm, h, p in _LINES)
PRIMARY_N = (1, 33, 2100)
SECONDARY_N = 1000


@functools.lru_cache(maxsize=None)
def fresh_net(layers, seed=5):
    rng = np.random.default_rng(seed)
    Ws, bs = po.xavier_init(list(layers), rng)
    bs = [0.3 * rng.standard_normal(b.shape) for b in bs]
    flat = po.pack_params(Ws, bs)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def golden_net(name):
    """(layers, flat) of tests/golden/weights_<name>.npz"""
    w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{name}.npz"))
    layers = [int(v) for v in w["layers"]]
    nl = len(layers) - 1
    flat = po.pack_params([w[f"W{i}"] for i in range(nl)], [w[f"b{i}"] for i in range(nl)])
    flat.setflags(write=False)
    return layers, flat


def _f32(X):
    X = np.asarray(X).astype(np.float32).astype(np.float64)        # (what the device sees)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def plate_uniform(n, seed=77):
    """uniform points of [0,0.5]^2 x [0,10] (primary check: the hole does not matter to the head's rounding)"""
    return _f32(np.random.default_rng(seed).random((n, 3)) * np.asarray(PLATE_UB))


@functools.lru_cache(maxsize=None)
def plate_set(n, seed=1111):
    """the plate's collocation sampler: the box minus the hole (golden_points.plate_points)"""
    return _f32(gp.plate_points(n=n, seed=seed))


@functools.lru_cache(maxsize=None)
def plate_frozen(n, seed=9):
    """random frozen D / P streams [2,5,5,n] with the scales of the plate's kernel tests (value 1, d/dx and d/dy 2, d/dt 0.2, d2/dt2 0.05), fp32"""
    rng = np.random.default_rng(seed)
    fr = (rng.standard_normal((2, 5, 5, n)) * np.array([1.0, 2.0, 2.0, 0.2, 0.05])[None, :, None, None]).astype(np.float32)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def nc3d_points(n, seed=77):
    """stratified points of the half-space box (nc3d_oracle.halfspace_points)"""
    return _f32(n3.halfspace_points(n, NC3D_LB, NC3D_UB, np.random.default_rng(seed)))


def _weighted(terms, w):
    s = np.zeros(terms[0][0].shape[-1])
    b = np.zeros_like(s)
    for wi, tt in zip(w, terms):
        s += wi * sum(tt) ** 2
        b += abs(wi) * sum(np.abs(v) for v in tt) ** 2
    return s, HEAD_C * EPS32 * b


def plate_score_from_streams(N, frozen, w=PLATE_WEIGHTS, E=20.0, mu=0.25, rho=1.0):
    """PRIMARY reference of pinn_plate2d_residual_score: composite and residual formulas (PLATE:383-387, 404-439) in float64 on the fp32 output
    N [5,5,n] of pinn_net_streams of the same mode and the fp32 frozen streams [2,5,5,n] that were passed in.  Returns (score [n], bound [n]);
    bound = C eps32 sum_i |w_i| a_i^2 with a_i the sum of the absolute values of the LEAF terms of f_i with their coefficients (every P, D*N,
    2*D*N).  C by counting roundings as _refine_cases.score_from_fields does: the longest path of a leaf is the one of 2*D3*N3 into f_u -- 2 in
    the product, 3 additions into F[4] (the two inside D4*N0 + 2*D3*N3 + D0*N4 and the += onto P), 1 for rho, 2 additions in f_u: 8 roundings,
    relative 8 eps of a_i; the square 2 x 8 + 1; the weight 1; the five-term sum 4: 22.  (The stress residuals are shorter: 1 + 2 into F[k], then
    the strain sum or the second Hooke term, the coefficient and the subtraction: 6.)  C = 24 as the issue sets it for both families."""
    N, fr = np.asarray(N, dtype=np.float64), np.asarray(frozen, dtype=np.float64)
    D, P = fr[0], fr[1]
    c1, c2, G = po.hooke_coeffs(E, mu, False)

    def F(k, o, c=1.0):
        if k == 0:
            leaves = [P[0, o], D[0, o] * N[0, o]]
        elif k < 4:
            leaves = [P[k, o], D[k, o] * N[0, o], D[0, o] * N[k, o]]
        else:
            leaves = [P[4, o], D[4, o] * N[0, o], 2.0 * D[3, o] * N[3, o], D[0, o] * N[4, o]]
        return [c * v for v in leaves]

    terms = [F(1, 2) + F(2, 4) + F(4, 0, -rho), F(2, 3) + F(1, 4) + F(4, 1, -rho),
             F(0, 2) + F(1, 0, -c1) + F(2, 1, -c2), F(0, 3) + F(1, 0, -c2) + F(2, 1, -c1), F(0, 4) + F(2, 0, -G) + F(1, 1, -G)]
    return _weighted(terms, w)


def nc3d_score_from_fields(Fd, w=NC3D_WEIGHTS, E=2.5, mu=0.25, rho=1.0):
    """PRIMARY reference of pinn_nc3d_residual_score: the twelve residual formulas (oracle/nc3d_oracle.py) in float64 on the fp32 output Fd
    [5,12,n] of pinn_nc3d_fields of the same mode.  bound = C eps32 sum_i |w_i| a_i^2; the longest path of a term is e_jj in a normal-stress
    residual -- e_jj + e_kk, the coefficient c2, the addition to c1 e_ii, the subtraction: 4 roundings (momentum: rho, 3 additions: 4), so
    2 x 4 + 1 + 1 + 11 = 21; C = 24 as the issue sets it."""
    Fd = np.asarray(Fd, dtype=np.float64)
    V, X, Y, Z, T = Fd
    c1, c2, G = n3.hooke3d(E, mu)
    terms = [(X[6], Y[9], Z[10], -rho * T[3]), (X[9], Y[7], Z[11], -rho * T[4]), (X[10], Y[11], Z[8], -rho * T[5]),
             (T[0], -V[3]), (T[1], -V[4]), (T[2], -V[5]),
             (V[6], -c1 * X[0], -c2 * Y[1], -c2 * Z[2]), (V[7], -c1 * Y[1], -c2 * X[0], -c2 * Z[2]), (V[8], -c1 * Z[2], -c2 * X[0], -c2 * Y[1]),
             (V[9], -G * Y[0], -G * X[1]), (V[10], -G * Z[0], -G * X[2]), (V[11], -G * Z[1], -G * Y[2])]
    return _weighted(terms, w)


# ---- secondary: the float64 oracle ---------------------------------------------------------------------------------------------------------------
def plate_oracle_score(flat, layers, X, w, dtype=np.float64, E=20.0, mu=0.25, rho=1.0):
    """net_streams of the uv net and of the trained distance / particular nets -> composite -> plate_residuals, all in `dtype`; squared and
    weighted in float64"""
    st = lambda f, l: pl.net_streams(np.asarray(f), list(l), X[:, 0], X[:, 1], X[:, 2], dtype=dtype)
    ld, fd = golden_net("plate_dist")
    lp, fp = golden_net("plate_part")
    F = pl.composite(st(flat, layers), st(fd, ld), st(fp, lp))
    f = pl.plate_residuals(F, dtype(E), dtype(mu), dtype(rho)).astype(np.float64)
    return (f ** 2) @ np.asarray(w, dtype=np.float64)


def nc3d_oracle_score(flat, layers, X, w, dtype=np.float64, E=2.5, mu=0.25, rho=1.0):
    out = n3.nc3d_fields(np.asarray(flat), list(layers), X[:, 0], X[:, 1], X[:, 2], X[:, 3], NC3D_LB, NC3D_UB, True, dtype=dtype)
    f = n3.nc3d_residuals(out["Y"], out["dY"], dtype(E), dtype(mu), dtype(rho)).astype(np.float64)
    return (f ** 2) @ np.asarray(w, dtype=np.float64)


PLATE_DEFAULT_W = (10.0,) * 5                      # PINN.refine_collocation's default
NC3D_DEFAULT_W = (5.0,) * 12                       # NavierCauchy3D's default (LOSS_LAYOUT_3D)
PLATE_SECONDARY = ("xavier4x32", "plate70", "plate64")
NC3D_SECONDARY = ("xavier3x32", "xavier10x128")


def plate_net(name):
    if name == "xavier4x32":
        layers = [3] + 4 * [32] + [5]
        return layers, fresh_net(tuple(layers))
    return golden_net("plate_uv" if name == "plate70" else "plate64_uv")


def nc3d_net(name):
    layers = [4] + (3 * [32] if name == "xavier3x32" else 10 * [128]) + [12]
    return layers, fresh_net(tuple(layers))


def _case(score, layers, flat, X, w):
    ref = score(flat, layers, X, w)
    s32 = score(flat.astype(np.float32), layers, X.astype(np.float32), w, dtype=np.float32)
    base = (rel_l2(s32, ref), rel_l2(np.sqrt(s32), np.sqrt(ref)))
    return layers, flat, X, ref, base


@functools.lru_cache(maxsize=None)
def plate_secondary_case(name):
    """(layers, flat, X, float64 score, metrics of the float32 oracle run): the bar is 6 x the float32 oracle's own error, per metric.  The D / P
    streams are those of the trained distance / particular nets in every case (weights_plate_dist / weights_plate_part)."""
    layers, flat = plate_net(name)
    return _case(plate_oracle_score, layers, flat, plate_set(SECONDARY_N, 1111), PLATE_DEFAULT_W)


@functools.lru_cache(maxsize=None)
def nc3d_secondary_case(name):
    layers, flat = nc3d_net(name)
    return _case(nc3d_oracle_score, layers, flat, nc3d_points(SECONDARY_N, 1111), NC3D_DEFAULT_W)
