"""Cases and references shared by the predict-head tests (test_emulated_predict.py, test_gpu_predict.py, test_predict_host.py): the two
references of pinn_wave2d_predict / pinn_plate2d_predict and the data of pinn_field_error_sums.  Everything here is
computed on the host; the references are built once per case (functools.lru_cache) and never written to.  Nets, points and frozen streams are
those of tests/_refine_cases.py and tests/_refine_family_cases.py."""
import functools

import numpy as np

from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests import _refine_cases as RC
from tests._refine_cases import EPS32, LB, UB, rel_l2  # noqa: F401
from tests._refine_family_cases import _LINES, PLATE_LB, PLATE_UB, fresh_net, golden_net, plate_frozen, plate_set, plate_uniform  # noqa: F401

HEAD_C = 4.0           # roundings of the predict heads, see *_from_* below
PRIMARY_N = (1, 33, 2100)
SECONDARY_N = 1000
GUARD = 64

# (name, layers, precision): every padded width in f16x3, the bf16 split mode, the fp32 checking mode; the wave head also the one-MFMA modes
WAVE_LINES = tuple((nm, [3] + h + [7], p) for nm, h, p in _LINES) + (("bf16", [3] + 3 * [64] + [7], "bf16"), ("f16", [3] + 3 * [64] + [7], "f16"))
PLATE_LINES = tuple((nm, [3] + h + [5], p) for nm, h, p in _LINES)

WAVE_ROWS = ("u", "v", "s11", "s22", "s12", "e11", "e22", "e12")
VALUE_ROWS = {"wave": slice(0, 5), "plate": slice(0, 5)}
STRAIN_ROWS = {"wave": slice(5, 8), "plate": slice(5, 8)}


class Guarded:
    """nbytes of payload at a 256-byte aligned address, guard words in front and behind (the emulator tests' host buffers)"""

    def __init__(self, nbytes, fill=0xA5):
        self.raw = np.full(nbytes + 2 * GUARD + 512, 0xA5, dtype=np.uint8)
        base = self.raw.ctypes.data
        self.off = (-(base + GUARD) % 256) + GUARD
        self.nbytes = nbytes
        self.ptr = base + self.off
        self.raw[self.off:self.off + nbytes] = fill

    def view(self, dtype):
        return self.raw[self.off:self.off + self.nbytes].view(dtype)

    def guards_intact(self):
        return bool((self.raw[:self.off] == 0xA5).all() and (self.raw[self.off + self.nbytes:] == 0xA5).all())


def put(a):
    a = np.ascontiguousarray(a)
    g = Guarded(a.nbytes)
    g.view(a.dtype)[:] = a.reshape(-1)
    return g


def wave_points(n):
    return RC.points(n)


def _rows(rows):
    """rows: list of leaf-term lists -> (value [R, n], bound [R, n]); bound = HEAD_C eps32 (sum of the absolute values of the leaves)"""
    ref = np.stack([sum(r) for r in rows])
    a = np.stack([sum(np.abs(v) for v in r) for r in rows])
    return ref, HEAD_C * EPS32 * a


# ---- primary references: the head's formulas in float64 on the fp32 output of the library's own fields / streams call ------------------------------
# The count behind HEAD_C = 4: the longest path is the plate's e12 -- two products and three additions inside an Fk, one more in the sum: at most six
# roundings of half an ulp each, relative to the leaves; a copied row has none.  The carried streams run the per-stream instructions of the
# fields call, so no slack is granted for the forward.
def wave_predict_from_fields(F):
    """F [4,7,n] of pinn_wave2d_fields -> ([8,n], bound): u, v, s11, s22, s12 = outputs 0, 1, 4, 5, 6; e11 = du/dx, e22 = dv/dy, e12 = du/dy + dv/dx"""
    F = np.asarray(F, dtype=np.float64)
    V, X, Y = F[0], F[1], F[2]
    return _rows([[V[0]], [V[1]], [V[4]], [V[5]], [V[6]], [X[0]], [Y[1]], [Y[0], X[1]]])


def plate_predict_from_streams(N, frozen):
    """N [5,5,n] of pinn_net_streams, frozen fp32 [2,5,5,n] (stream rows 0..2 used) -> ([8,n], bound):
    F0 = P0 + D0 N0, Fk = Pk + Dk N0 + D0 Nk; rows F0[u], F0[v], F0[s11], F0[s22], F0[s12], F1[u], F2[v], F2[u] + F1[v]"""
    N = np.asarray(N, dtype=np.float64)
    D, P = np.asarray(frozen[0][:3], dtype=np.float64), np.asarray(frozen[1][:3], dtype=np.float64)
    F0 = lambda o: [P[0, o], D[0, o] * N[0, o]]
    Fk = lambda k, o: [P[k, o], D[k, o] * N[0, o], D[0, o] * N[k, o]]
    return _rows([F0(0), F0(1), F0(2), F0(3), F0(4), Fk(1, 0), Fk(2, 1), Fk(2, 0) + Fk(1, 1)])


def poisoned(frozen):
    """the frozen streams with stream rows 3 and 4 of both blocks set to NaN: the predict head must not read them"""
    fr = np.array(frozen, dtype=np.float32)
    fr[:, 3:, :, :] = np.nan
    fr.setflags(write=False)
    return fr


# ---- secondary references: the float64 formulas of the reference classes ------------------------------------------------------------------------------
def wave_reference(flat, layers, X, dtype=np.float64):
    o = po.wave2d_fields(np.asarray(flat), list(layers), X[:, 0], X[:, 1], X[:, 2], LB, UB, True, dtype=dtype)
    return np.stack([o[k] for k in WAVE_ROWS]).astype(np.float64)


def plate_reference(flat, layers, X, dtype=np.float64):
    st = lambda f, l: pl.net_streams(np.asarray(f), list(l), X[:, 0], X[:, 1], X[:, 2], dtype=dtype)
    ld, fd = golden_net("plate_dist")
    lp, fp = golden_net("plate_part")
    F = pl.composite(st(flat, layers), st(fd, ld), st(fp, lp))
    return np.stack([F[0, 0], F[0, 1], F[0, 2], F[0, 3], F[0, 4], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]]).astype(np.float64)


def block_errors(family, out, ref):
    """(relative L2 of the value rows as one block, of the strain rows as one block)"""
    out = np.asarray(out, dtype=np.float64)
    return rel_l2(out[VALUE_ROWS[family]], ref[VALUE_ROWS[family]]), rel_l2(out[STRAIN_ROWS[family]], ref[STRAIN_ROWS[family]])


SECONDARY = {"wave": ("xavier4x32", "xavier8x64", "inf20s"), "plate": ("xavier4x32", "plate70", "plate64")}
SECONDARY_CASES = tuple((fam, net) for fam in ("wave", "plate") for net in SECONDARY[fam])


def _net(family, name):
    if family == "wave":
        if name == "inf20s":
            return RC.trained_net()
        layers = [3] + (4 * [32] if name == "xavier4x32" else 8 * [64]) + [7]
    else:
        if name != "xavier4x32":
            return golden_net("plate_uv" if name == "plate70" else "plate64_uv")
        layers = [3] + 4 * [32] + [5]
    return layers, fresh_net(tuple(layers))


@functools.lru_cache(maxsize=None)
def secondary_case(family, name):
    """(layers, flat, X, float64 reference [rows, n], block errors of the float32 run of the reference): the bar is 6 x the latter, per block"""
    layers, flat = _net(family, name)
    X = {"wave": RC.collocation_set, "plate": plate_set}[family](SECONDARY_N, 1111)
    fn = {"wave": wave_reference, "plate": plate_reference}[family]
    ref = fn(flat, layers, X)
    base = block_errors(family, fn(flat.astype(np.float32), layers, X.astype(np.float32), dtype=np.float32), ref)
    ref.setflags(write=False)
    return layers, flat, X, ref, base


# ---- pinn_field_error_sums ---------------------------------------------------------------------------------------------------------------------------------
ERR_N = (0, 1, 33, 2100, 70001)          # the last spans several workgroups
ERR_PRED_ROWS = 8
ERR_ROWS = (0, 1, 4)


@functools.lru_cache(maxsize=None)
def error_data(n):
    """(pred fp32 [8, n] with NaN in the rows that are not selected, ref fp32 [3, n], float64 sums [2, 3] by numpy on the same fp32 arrays)"""
    rng = np.random.default_rng(4000 + n)
    pred = np.full((ERR_PRED_ROWS, n), np.nan, dtype=np.float32)
    scale = np.array([[1.0], [1e-3], [50.0]])
    ref = (rng.standard_normal((len(ERR_ROWS), n)) * scale).astype(np.float32)
    for j, r in enumerate(ERR_ROWS):
        pred[r] = ref[j] + (0.05 * scale[j, 0] * rng.standard_normal(n)).astype(np.float32)
    p64, r64 = pred[list(ERR_ROWS)].astype(np.float64), ref.astype(np.float64)
    sums = np.stack([((p64 - r64) ** 2).sum(1), (r64 ** 2).sum(1)])
    for a in (pred, ref, sums):
        a.setflags(write=False)
    return pred, ref, sums
