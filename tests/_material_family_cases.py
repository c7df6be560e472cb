"""Cases and references shared by the material-identification tests of the plate and 3-D families (test_emulated_material_families.py,
test_gpu_material_families.py, test_material_families_host.py): the float64 reference of the 12 sums of pinn_plate2d_material_sums from a
streams array and of the 24 sums of pinn_nc3d_material_sums from a fields array, the bound of each head's own rounding, the float64 oracle's
sums and a CPU stand-in engine that serves them.  Points, nets and frozen streams are those of tests/_refine_family_cases.py; everything here
is computed on the host, the cached references are never written to."""
import functools

import numpy as np
import torch

from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests import _refine_family_cases as FC
from tests._material_cases import scaled_error  # noqa: F401
from tests._oracle_engine import OracleEngine

EPS32 = FC.EPS32
PLATE_LINES, NC3D_LINES, PRIMARY_N, SECONDARY_N = FC.PLATE_LINES, FC.NC3D_LINES, FC.PRIMARY_N, FC.SECONDARY_N
PLATE_SECONDARY, NC3D_SECONDARY = FC.PLATE_SECONDARY, FC.NC3D_SECONDARY
PLATE_NSUMS, NC3D_NSUMS = 12, 24
PLATE_CONSTS, NC3D_CONSTS = (20.0, 0.25, 1.0), (2.5, 0.25, 1.0)          # the classes' constants
GENERAL = (7.3, 0.31, 1.9)
# Rounding counts of the heads.  Plate: the longest residual path is the 8 roundings plate_score_from_streams counts (2*D3*N3 into f_u) + 1
# for the fp32 coefficient: a square 2 x 9 = 18, a moment 9 + 4 (the composite strain: product, two additions into F[k], the strain sum)
# = 13; C = 24, the families' HEAD_C.  3-D: 4 + 1 roundings in a residual: a square 10, a moment 5 + 1 (the pair sum or the shear sum); C = 12.
PLATE_C, NC3D_C = FC.HEAD_C, 12.0


def _reduce(terms, pairs, C):
    """terms[i]: the leaf terms of f_i (arrays [n]); pairs: (i, leaves of the second factor g).  Returns (sums, bound, scale) with
    scale = sum_n a_i^2 for the squares, sum_n a_i |g| for the moments (a_i, |g| the leaf-wise absolute sums), bound = C eps32 scale."""
    f = [sum(tt) for tt in terms]
    a = [sum(np.abs(v) for v in tt) for tt in terms]
    sums = [float((fi * fi).sum()) for fi in f] + [float((f[i] * sum(g)).sum()) for i, g in pairs]
    scale = np.asarray([float((ai * ai).sum()) for ai in a] + [float((a[i] * sum(np.abs(v) for v in g)).sum()) for i, g in pairs])
    return np.asarray(sums), C * EPS32 * scale, scale


def plate_sums_from_streams(N, frozen, E=20.0, mu=0.25, rho=1.0):
    """PRIMARY reference of pinn_plate2d_material_sums: composite and residual formulas (PLATE:383-387, 404-439) in float64, with float64
    coefficients, on the fp32 output N [5,5,n] of pinn_net_streams of the same mode and the fp32 frozen streams [2,5,5,n] that were passed in.
    Leaves as in _refine_family_cases.plate_score_from_streams: every P, D*N, 2*D*N with its coefficient.  Returns (sums [12], bound, scale)."""
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
    e11, e22, e12 = F(1, 0), F(2, 1), F(2, 0) + F(1, 1)
    pairs = [(2, e11), (2, e22), (3, e11), (3, e22), (4, e12), (0, F(4, 0)), (1, F(4, 1))]
    return _reduce(terms, pairs, PLATE_C)


def nc3d_sums_from_fields(Fd, E=2.5, mu=0.25, rho=1.0):
    """PRIMARY reference of pinn_nc3d_material_sums: the twelve residual formulas (oracle/nc3d_oracle.py) in float64 on the fp32 output Fd
    [5,12,n] of pinn_nc3d_fields of the same mode; leaves as in _refine_family_cases.nc3d_score_from_fields.  Returns (sums [24], bound, scale)."""
    Fd = np.asarray(Fd, dtype=np.float64)
    V, X, Y, Z, T = Fd
    c1, c2, G = n3.hooke3d(E, mu)
    terms = [(X[6], Y[9], Z[10], -rho * T[3]), (X[9], Y[7], Z[11], -rho * T[4]), (X[10], Y[11], Z[8], -rho * T[5]),
             (T[0], -V[3]), (T[1], -V[4]), (T[2], -V[5]),
             (V[6], -c1 * X[0], -c2 * Y[1], -c2 * Z[2]), (V[7], -c1 * Y[1], -c2 * X[0], -c2 * Z[2]), (V[8], -c1 * Z[2], -c2 * X[0], -c2 * Y[1]),
             (V[9], -G * Y[0], -G * X[1]), (V[10], -G * Z[0], -G * X[2]), (V[11], -G * Z[1], -G * Y[2])]
    pairs = [(6, [X[0]]), (6, [Y[1], Z[2]]), (7, [Y[1]]), (7, [X[0], Z[2]]), (8, [Z[2]]), (8, [X[0], Y[1]]),
             (9, [Y[0], X[1]]), (10, [Z[0], X[2]]), (11, [Z[1], Y[2]]), (0, [T[3]]), (1, [T[4]]), (2, [T[5]])]
    return _reduce(terms, pairs, NC3D_C)


# ---- secondary: the float64 oracle ---------------------------------------------------------------------------------------------------------------
def _moments(f, factors, pairs):
    """f [n, k] residuals, factors: arrays [n]; squares and products in float64"""
    f = np.asarray(f, dtype=np.float64)
    return np.asarray([float((f[:, i] ** 2).sum()) for i in range(f.shape[1])]
                      + [float((f[:, i] * np.asarray(factors[j], dtype=np.float64)).sum()) for i, j in pairs])


def plate_sums_of_composite(F, E, mu, rho):
    """the 12 sums from composite streams F [5,5,n] in F's dtype: plate_oracle.plate_residuals, factors from F, products and sums in float64"""
    dt = F.dtype.type
    f = pl.plate_residuals(F, dt(E), dt(mu), dt(rho))
    fac = [F[1, 0], F[2, 1], F[2, 0] + F[1, 1], F[4, 0], F[4, 1]]
    return _moments(f, fac, [(2, 0), (2, 1), (3, 0), (3, 1), (4, 2), (0, 3), (1, 4)])


def nc3d_sums_of_fields(Y, dY, E, mu, rho):
    """the 24 sums from the oracle's fields (Y [n,12], dY four of [n,12]) in their dtype: nc3d_oracle.nc3d_residuals, products and sums in float64"""
    dt = Y.dtype.type
    f = n3.nc3d_residuals(Y, dY, dt(E), dt(mu), dt(rho))
    Jx, Jy, Jz, Jt = dY
    e11, e22, e33 = Jx[:, 0], Jy[:, 1], Jz[:, 2]
    fac = [e11, e22 + e33, e22, e11 + e33, e33, e11 + e22, Jy[:, 0] + Jx[:, 1], Jz[:, 0] + Jx[:, 2], Jz[:, 1] + Jy[:, 2], Jt[:, 3], Jt[:, 4], Jt[:, 5]]
    return _moments(f, fac, [(6, 0), (6, 1), (7, 2), (7, 3), (8, 4), (8, 5), (9, 6), (10, 7), (11, 8), (0, 9), (1, 10), (2, 11)])


def plate_oracle_sums(flat, layers, X, consts=PLATE_CONSTS, dtype=np.float64):
    """the oracle's own forward in `dtype`: net_streams of the uv net and of the trained distance / particular nets -> composite -> sums.
    Returns (sums, scale); the scale is the one of plate_sums_from_streams on the same streams."""
    st = lambda f, l: pl.net_streams(np.asarray(f), list(l), X[:, 0], X[:, 1], X[:, 2], dtype=dtype)
    ld, fd = FC.golden_net("plate_dist")
    lp, fp = FC.golden_net("plate_part")
    N, D, P = st(flat, layers), st(fd, ld), st(fp, lp)
    return plate_sums_of_composite(pl.composite(N, D, P), *consts), plate_sums_from_streams(N, np.stack([D, P]), *consts)[2]


def nc3d_oracle_sums(flat, layers, X, consts=NC3D_CONSTS, dtype=np.float64):
    out = n3.nc3d_fields(np.asarray(flat), list(layers), X[:, 0], X[:, 1], X[:, 2], X[:, 3], FC.NC3D_LB, FC.NC3D_UB, True, dtype=dtype)
    Fd = np.stack([out["Y"].T] + [d.T for d in out["dY"]])
    return nc3d_sums_of_fields(out["Y"], out["dY"], *consts), nc3d_sums_from_fields(Fd, *consts)[2]


def _case(oracle_sums, layers, flat, X):
    ref, scale = oracle_sums(flat, layers, X)
    s32, _ = oracle_sums(flat.astype(np.float32), layers, X.astype(np.float32), dtype=np.float32)
    return layers, flat, X, ref, scale, scaled_error(s32, ref, scale)


@functools.lru_cache(maxsize=None)
def plate_secondary_case(name):
    """(layers, flat, X, float64 oracle sums, scale, metric of the float32 oracle run): the bar is 6 x the float32 oracle's own error.  The D / P
    streams are those of the trained distance / particular nets in every case."""
    layers, flat = FC.plate_net(name)
    return _case(plate_oracle_sums, layers, flat, FC.plate_set(SECONDARY_N, 1111))


@functools.lru_cache(maxsize=None)
def nc3d_secondary_case(name):
    layers, flat = FC.nc3d_net(name)
    return _case(nc3d_oracle_sums, layers, flat, FC.nc3d_points(SECONDARY_N, 1111))


def tiles_n():
    """the smallest n at which a wave of the five-stream chain grid walks a second tile: Host::MAX_BLOCKS workgroups of 4 waves, one tile of
    16 * nb<5>() points each, + 1.  MAX_BLOCKS and the tile are read from the library's constants: the sums workspace holds MAX_BLOCKS * 4
    records of 24 doubles, and a five-stream tile is 16 points (nb<5>() = 1; the four-stream tile of the wave test is 32)."""
    from pinn_elastodynamics_amd.capi import PinnLib
    records = PinnLib().material_sums_workspace_bytes() // (NC3D_NSUMS * 8)
    return records * 16 + 1


class FamilyMaterialEngine(OracleEngine):
    """OracleEngine + plate_material_sums / nc3d_material_sums from the float64 oracle on the streams the stand-in itself returns, and a call
    log of the collocation evaluations (the CPU side of the identification tests)"""

    def for_layers(self, layers):
        return FamilyMaterialEngine(layers)

    def plate_loss_grad(self, params, x, *a, **kw):
        self.calls.append(("plate", x.numel()))
        return super().plate_loss_grad(params, x, *a, **kw)

    def nc3d_loss_grad(self, params, x, *a, **kw):
        self.calls.append(("nc3d", x.numel()))
        return super().nc3d_loss_grad(params, x, *a, **kw)

    @staticmethod
    def _out(s, out):
        if out is None:
            out = torch.zeros(s.size, dtype=torch.float64)
        out.copy_(torch.from_numpy(s))
        return out

    def plate_material_sums(self, params, x, y, t, lb, ub, normalize, frozen, E, mu, rho, out=None, packed=False):
        self.calls.append(("material", x.numel(), bool(packed)))
        fr = self._np(frozen)
        assert fr.shape == (2, 5, 5, x.numel())
        N = pl.net_streams(self._np(params), self.layers, self._np(x), self._np(y), self._np(t))
        return self._out(plate_sums_of_composite(pl.composite(N, fr[0], fr[1]), E, mu, rho), out)

    def nc3d_material_sums(self, params, x, y, z, t, lb, ub, normalize, E, mu, rho, out=None, packed=False):
        self.calls.append(("material", x.numel(), bool(packed)))
        o = n3.nc3d_fields(self._np(params), self.layers, self._np(x), self._np(y), self._np(z), self._np(t), lb, ub, normalize)
        return self._out(nc3d_sums_of_fields(o["Y"], o["dY"], E, mu, rho), out)
