"""Cases shared by the grid-cap tests (test_gpu_grid_caps.py, test_emulated_grid_caps.py): every kernel outside the fused training step launches a
CAPPED grid in which a workgroup (or a wave) owns a contiguous index range or a strided list of tiles.  Below the cap each of them sees one tile
and the loop that carries state from one tile to the next never runs; the sizes here are the first at which it does.

The caps are READ from the sources (constexpr int NAME = <int>, as _variant_matrix.py reads pinn_variants.def), every size is derived from them as
cap_points + 1 and 2 * cap_points + tile + 1 (a third trip for some workgroups, a ragged last one), and test_sizes_exceed_the_caps_read_from_the_
sources holds the derived numbers to today's table -- whoever raises a cap has to look at this file.  Data, references and bars are those of the
existing case modules (_refine_cases, _refine_family_cases, _predict_cases, _causal_cases, _variant_matrix); nothing here was taken from a
device's output."""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

from oracle import nc3d_oracle as n3
from oracle import pinn_oracle as po
from oracle import plate_oracle as pl
from tests import _causal_cases as CC
from tests import _predict_cases as PC
from tests import _refine_cases as RC
from tests import _refine_family_cases as FC
from tests import _variant_matrix as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc")
NB_RULE = "static constexpr int nb() { return (WIDTH <= 64 && NS != 5) ? 2 : 1; }"
FP32_RULE = "return ((size_t)2 * (net.nl + 1) * ns * hr + FP32_TERMS) * sizeof(float);"
WAVES_PER_WORKGROUP, POINTS_PER_BLOCK = 4, 16      # chain_kernel: 256 threads, one 16-point MFMA block (NB of them) per wave and tile


@functools.lru_cache(maxsize=None)
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(header, name):
    """the one `constexpr int NAME = <int>` of a header (each of these headers holds one namespace, or one Host template)"""
    found = re.findall(r"constexpr int %s = (\d+)\s*;" % re.escape(name), _source(header))
    assert len(found) == 1, f"{header}: expected one 'constexpr int {name} = <int>', found {len(found)} -- tests/_grid_cap_cases.py reads the cap there"
    return int(found[0])


def _require(header, text):
    assert text in _source(header), f"{header} no longer holds '{text}': the sizes of tests/_grid_cap_cases.py are derived from that rule, look at both"


# ---- the caps -----------------------------------------------------------------------------------------------------------------------------------
HOST_MAX_BLOCKS = constant("pinn_host.hpp", "MAX_BLOCKS")
NB_PREDICT = constant("pinn_host.hpp", "NB_PREDICT")
CAUSAL_MAX_BLOCKS, CAUSAL_TILE = constant("pinn_causal.hpp", "MAX_BLOCKS"), constant("pinn_causal.hpp", "TILE")
VALIDATE_MAX_BLOCKS, VALIDATE_TILE = constant("pinn_validate.hpp", "MAX_BLOCKS"), constant("pinn_sample.hpp", "THREADS")      # (validate::THREADS = sample::THREADS)
SELECT_MAX_BLOCKS, SELECT_TILE = constant("pinn_select.hpp", "MAX_BLOCKS"), constant("pinn_select.hpp", "THREADS")
FP32_TERMS, FP32_MAX_NS = constant("pinn_fp32.hpp", "FP32_TERMS"), constant("pinn_fp32.hpp", "FP32_MAX_NS")
_require("pinn_validate.hpp", "constexpr int THREADS = sample::THREADS;")


def nb(width, ns, predict=False):
    """blocks per wave of a forward head's chain launch: Host::nb<NS>() (the text is held in place), NB_PREDICT for the predict heads"""
    _require("pinn_host.hpp", NB_RULE)
    return NB_PREDICT if predict else (2 if width <= 64 and ns != 5 else 1)


def sizes(cap_points, tile):
    return cap_points + 1, 2 * cap_points + tile + 1


def chain_cap(nblocks):
    """(points the capped chain grid covers in one trip per wave, points per wave tile)"""
    tile = POINTS_PER_BLOCK * nblocks
    return HOST_MAX_BLOCKS * WAVES_PER_WORKGROUP * tile, tile


def ranges(n, max_blocks, tile):
    """(workgroups, indices per workgroup) as the launch() of pinn_select.hpp, pinn_validate.hpp and launch_bins() of pinn_causal.hpp compute them"""
    blocks = min(max((n + tile - 1) // tile, 1), max_blocks)
    per = (n + blocks - 1) // blocks
    return blocks, (per + tile - 1) // tile * tile


BINNED_CAP, FIELD_ERR_CAP, SELECT_CAP = CAUSAL_MAX_BLOCKS * CAUSAL_TILE, VALIDATE_MAX_BLOCKS * VALIDATE_TILE, SELECT_MAX_BLOCKS * SELECT_TILE
BINNED_N, FIELD_ERR_N, SELECT_N = sizes(BINNED_CAP, CAUSAL_TILE), sizes(FIELD_ERR_CAP, VALIDATE_TILE), sizes(SELECT_CAP, SELECT_TILE)


# ---- chain forward heads ----------------------------------------------------------------------------------------------------------------------
# head -> (family, streams, predict head?, output rows per point)
HEADS = {"wave_fields": ("wave", 4, False, 28), "wave_score": ("wave", 4, False, 1), "wave_predict": ("wave", 3, True, 8),
         "net_streams": ("plate", 5, False, 25), "plate_score": ("plate", 5, False, 1), "plate_predict": ("plate", 3, True, 8),
         "nc3d_fields": ("nc3d", 5, False, 60), "nc3d_score": ("nc3d", 5, False, 1)}
NOUT = {"wave": 7, "plate": 5, "nc3d": 12}
FIELDS_OF = {"wave_score": "wave_fields", "wave_predict": "wave_fields", "plate_score": "net_streams", "plate_predict": "net_streams",
             "nc3d_score": "nc3d_fields"}
FP32_MAX_POINTS = 1 << 13          # the engines of the refinement and predict tests


@dataclass(frozen=True)
class Row:
    head: str
    hidden: int
    prec: str
    big: bool = False          # 2 * cap_points + tile + 1 instead of cap_points + 1

    @property
    def family(self):
        return HEADS[self.head][0]

    @property
    def ns(self):
        return HEADS[self.head][1]

    @property
    def rows(self):
        return HEADS[self.head][3]

    @property
    def layers(self):
        return [4 if self.family == "nc3d" else 3] + 2 * [self.hidden] + [NOUT[self.family]]

    @property
    def width(self):
        return next(w for w in vm.WIDTHS if self.hidden <= w)

    @property
    def cap(self):
        """(cap_points, tile) of this row's launch: the capped chain grid, or a workspace pass of the fp32 mode"""
        if self.prec == "fp32":
            return fp32_pass_points(self.layers, self.ns, fp32_workspace_bytes(self.layers)), 1
        return chain_cap(nb(self.width, self.ns, HEADS[self.head][2]))

    @property
    def n(self):
        if self.prec == "fp32":
            return 70001
        return sizes(*self.cap)[1 if self.big else 0]

    def __str__(self):
        return f"{self.head}-w{self.hidden}-{self.prec}-{self.n}"


def fp32_bytes_per_point(layers, ns):
    """fp32_bytes_per_point of pinn_fp32.hpp (the text is held in place)"""
    _require("pinn_fp32.hpp", FP32_RULE)
    return (2 * (len(layers) - 1) * ns * max(layers[1], 16) + FP32_TERMS) * 4


def fp32_workspace_bytes(layers, max_points=FP32_MAX_POINTS):
    """pinn_workspace_bytes in PINN_PREC_FP32 (pinn_capi.hip) for 256 <= max_points <= 65536"""
    return (fp32_bytes_per_point(layers, FP32_MAX_NS) * max_points + 255) // 256 * 256


def fp32_pass_points(layers, ns, ws_bytes):
    """mmax of fp32_call (pinn_capi.hip): the points of one workspace pass"""
    _require("pinn_capi.hip", "long mmax = (long)(c.ws_bytes / per_point);")
    return min(ws_bytes // fp32_bytes_per_point(layers, ns), 1 << 20)


def _rows(hidden, prec, heads, big=False):
    return [Row(h, hidden, prec, big) for h in heads.split()]


# the issue's table: width 64 is NB = 2 for the four-stream wave heads, width 100 (padded 128) NB = 1; the predict heads and the five-stream heads
# NB = 1 at every width; the 4-input kernels at width 100; one bf16 line for the wave heads at width 64; the larger size for one wave row (with its
# score) and one five-stream row
SPLIT_ROWS = (_rows(64, "f16x3", "wave_fields wave_score wave_predict") + _rows(100, "f16x3", "wave_fields wave_score wave_predict")
              + _rows(64, "f16x3", "net_streams plate_score plate_predict") + _rows(100, "f16x3", "nc3d_fields nc3d_score")
              + _rows(64, "bf16", "wave_fields wave_score wave_predict")
              + _rows(64, "f16x3", "wave_fields wave_score", big=True) + _rows(64, "f16x3", "net_streams", big=True))
FP32_ROWS = (_rows(64, "fp32", "wave_fields wave_score wave_predict net_streams plate_score plate_predict")
             + _rows(100, "fp32", "nc3d_fields nc3d_score"))
# what each row is held to.  The float64 oracle bars exist for f16x3 and fp32 only where they are "6 x the float32 oracle" (scores, predict:
# tests/test_gpu_refine.py, test_gpu_predict.py run them in those two modes); the one-MFMA bf16 mode is held to them for the fields (BAR["bf16"])
# and to the PRIMARY references for score and predict, as RC.PRIMARY_LINES and PC.WAVE_LINES hold it below the cap.
ORACLE_MODES = ("f16x3", "fp32")


def points(row):
    """float64 [n, din] of fp32-representable points, by the existing builders"""
    if row.family == "wave":
        return RC.points(row.n)
    if row.family == "plate":
        return FC.plate_set(row.n)
    return FC.nc3d_points(row.n)


def net(row):
    return FC.fresh_net(tuple(row.layers))


def frozen(row):
    return FC.plate_frozen(row.n) if row.family == "plate" else None


SUBSET_SEED = 20


@functools.lru_cache(maxsize=None)
def subset(n, cap_points, seed=SUBSET_SEED):
    """sorted indices: the first 64 points, the 64 on either side of cap_points, the last 64 (the ragged tile), 1024 random ones"""
    rng = np.random.default_rng(seed + n)
    idx = np.concatenate([np.arange(64), np.arange(cap_points - 64, cap_points + 64), np.arange(n - 64, n), rng.integers(0, n, 1024)])
    idx = np.unique(idx[(idx >= 0) & (idx < n)])
    idx.setflags(write=False)
    return idx


def _plate_F(flat, layers, X, fr, dtype):
    N = pl.net_streams(np.asarray(flat), list(layers), X[:, 0], X[:, 1], X[:, 2], dtype=dtype)
    return pl.composite(N, fr[0].astype(dtype), fr[1].astype(dtype))


def oracle(row, idx, dtype=np.float64):
    """the head's float64 (or float32) oracle at the points `idx` of the row's set, in the layout of the head's output [rows, len(idx)]"""
    L, flat, X = row.layers, net(row), points(row)[idx]
    if dtype is np.float32:
        flat, X = flat.astype(np.float32), X.astype(np.float32)
    fr = None if row.family != "plate" else np.asarray(frozen(row))[..., idx]
    h = row.head
    if h == "wave_fields":
        f = po.wave2d_fields(flat, L, X[:, 0], X[:, 1], X[:, 2], RC.LB, RC.UB, True, dtype=dtype)
        out = np.concatenate([f["Y"].T] + [d.T for d in f["dY"]])
    elif h == "wave_score":
        out = RC.oracle_score(flat, L, X, dtype=dtype)[None]
    elif h == "wave_predict":
        out = PC.wave_reference(flat, L, X, dtype=dtype)
    elif h == "net_streams":
        out = pl.net_streams(flat, L, X[:, 0], X[:, 1], X[:, 2], dtype=dtype).reshape(25, -1)
    elif h == "plate_score":
        f = pl.plate_residuals(_plate_F(flat, L, X, fr, dtype), dtype(20.0), dtype(0.25), dtype(1.0)).astype(np.float64)
        out = ((f ** 2) @ np.asarray(FC.PLATE_WEIGHTS, dtype=np.float64))[None]
    elif h == "plate_predict":
        F = _plate_F(flat, L, X, fr, dtype)
        out = np.stack([F[0, 0], F[0, 1], F[0, 2], F[0, 3], F[0, 4], F[1, 0], F[2, 1], F[2, 0] + F[1, 1]])
    elif h == "nc3d_fields":
        f = n3.nc3d_fields(flat, L, X[:, 0], X[:, 1], X[:, 2], X[:, 3], FC.NC3D_LB, FC.NC3D_UB, True, dtype=dtype)
        out = np.concatenate([f["Y"].T] + [d.T for d in f["dY"]])
    else:
        out = FC.nc3d_oracle_score(flat, L, X, FC.NC3D_WEIGHTS, dtype=dtype)[None]
    return np.asarray(out, dtype=np.float64)


def metrics(row, got, ref):
    """the existing metric of the head: relative L2 (fields, streams); (s, sqrt(s)) relative L2 (scores); (value rows, strain rows) (predict)"""
    got = np.asarray(got, dtype=np.float64)
    if row.head.endswith("score"):
        return RC.rel_l2(got, ref), RC.rel_l2(np.sqrt(got), np.sqrt(ref))
    if row.head.endswith("predict"):
        return PC.block_errors(row.family, got, ref)
    return (vm.rel(got, ref),)


@functools.lru_cache(maxsize=None)
def oracle_case(row):
    """(idx, float64 oracle [rows, len(idx)], bars): BAR[prec] for fields and streams; 6 x the float32 oracle's own error on the same subset for
    scores and predict, per metric"""
    idx = subset(row.n, row.cap[0])
    ref = oracle(row, idx)
    if row.head.endswith("score") or row.head.endswith("predict"):
        base = metrics(row, oracle(row, idx, np.float32), ref)
        bars = tuple(6.0 * b for b in base)
    else:
        bars = (vm.BAR[row.prec],)
    ref.setflags(write=False)
    return idx, ref, bars


def primary(row, F, fr=None):
    """(reference [rows, n], bound [rows, n]) of a score or predict row from the fp32 output F of the fields / streams call of the same mode at the
    same n: the helpers of the existing case modules"""
    if row.head == "wave_score":
        s, b = RC.score_from_fields(F)
    elif row.head == "plate_score":
        s, b = FC.plate_score_from_streams(F, fr)
    elif row.head == "nc3d_score":
        s, b = FC.nc3d_score_from_fields(F)
    elif row.head == "wave_predict":
        return PC.wave_predict_from_fields(F)
    else:
        return PC.plate_predict_from_streams(F, fr)
    return s[None], b[None]


# ---- pinn_binned_sums -------------------------------------------------------------------------------------------------------------------------
BINNED_BINS = (7, 64)


@functools.lru_cache(maxsize=None)
def binned_case(n, planted):
    """(value, coord) of _causal_cases.sums_case(n) -- edges, outsiders, NaN, +-inf and a negative are in it (five skipped points).  planted: in
    addition a skipped value and a NaN coordinate among the last three points (n - 3, n - 1) and at the cap: the NaN coordinate on index BINNED_CAP,
    the first point of the range behind the cap, the skipped value two in front of it (n - 2 holds sums_case's +inf).  At n = BINNED_CAP + 1 the two
    pairs are the same points, and the lone point of workgroup 256 is then a skipped one -- which is why the unplanted case runs too: there it COUNTS."""
    value, coord = (a.copy() for a in CC.sums_case(n))
    if planted:
        value[n - 3], coord[n - 1] = -2.0, np.nan
        value[BINNED_CAP - 2], coord[BINNED_CAP] = -2.0, np.nan
    for a in (value, coord):
        a.setflags(write=False)
    return value, coord


@functools.lru_cache(maxsize=None)
def binned_reference(n, planted, n_bins):
    return CC.binned_reference(*binned_case(n, planted), CC.LO, CC.HI, n_bins)


# ---- pinn_field_error_sums ----------------------------------------------------------------------------------------------------------------------
ERR_PRED_ROWS = 20
MAX_ROWS = constant("pinn_validate.hpp", "MAX_ROWS")


@functools.lru_cache(maxsize=None)
def error_case(n, n_rows):
    """(rows, pred fp32 [20, n] with NaN in the rows that are not selected, ref fp32 [n_rows, n], float64 sums [2, n_rows] by numpy on the same
    fp32 arrays) as _predict_cases.error_data builds them; rows: a permuted choice of n_rows of the 20"""
    rng = np.random.default_rng(4100 + n + n_rows)
    rows = tuple(int(r) for r in rng.permutation(ERR_PRED_ROWS)[:n_rows])
    scale = 10.0 ** rng.integers(-3, 3, (n_rows, 1))
    pred = np.full((ERR_PRED_ROWS, n), np.nan, dtype=np.float32)
    ref = (rng.standard_normal((n_rows, n)) * scale).astype(np.float32)
    sums = np.zeros((2, n_rows))
    for j, r in enumerate(rows):
        pred[r] = ref[j] + (0.05 * scale[j, 0] * rng.standard_normal(n)).astype(np.float32)
        p64, r64 = pred[r].astype(np.float64), ref[j].astype(np.float64)
        sums[0, j], sums[1, j] = ((p64 - r64) ** 2).sum(), (r64 ** 2).sum()
    for a in (pred, ref, sums):
        a.setflags(write=False)
    return rows, pred, ref, sums


ERR_CASES = tuple((n, r) for n in FIELD_ERR_N for r in (MAX_ROWS, 1))


# ---- pinn_select_k ------------------------------------------------------------------------------------------------------------------------------
SELECT_KINDS = ("equal", "ties", "top24", "special")


def tie_k(score, largest, n):
    """a k whose threshold falls among equals in the SECOND tile of a workgroup's range: the threshold is the key at index chunk + 299 (chunk as
    launch() computes it), k = the keys beyond it + its equals up to that index -- `need` then runs out at thread 43 of the second tile of
    workgroup 1.  For "equal" that is k = chunk + 300."""
    _, chunk = ranges(n, SELECT_MAX_BLOCKS, SELECT_TILE)
    assert chunk >= 2 * SELECT_TILE and chunk + 300 < n
    key = RC.keys_of(score)
    thr = key[chunk + 299]
    beyond = int((key > thr).sum() if largest else (key < thr).sum())
    return beyond + int((key[:chunk + 300] == thr).sum())


def select_ks(kind, n, largest):
    return sorted(set(RC.select_ks(n)) | {tie_k(RC.select_data(kind, n), largest, n), n - 1})
