"""CPU: the argument contract of the 18 single-set per-point entry points -- which PINN_ERR_* code every bad argument combination gets, and
therefore the ORDER of the checks (PINN_ERR_NULL for params / workspace before PINN_ERR_SIZE, then the point columns and the box, the
precision word, the layer list, the entry's own pointers, the output count, the sums workspace).  The expected codes
(tests/_capi_errors_parent.py) were recorded from the build before the entry points were folded into one table-driven helper and are not
regenerated.  The emulator library replays every case (the valid ones run their kernels on 16 points); the gfx950 library replays the cases
that answered with a negative code, which return before any HIP call and so need no GPU."""
import ctypes as C

import numpy as np

from pinn_elastodynamics_amd.capi import PREC, PROTOTYPES
from tests import _capi_errors_parent as parent
from tests.test_capi_symbols import lib  # noqa: F401  (the gfx950 library: its host-only paths run without a GPU)
from tests.test_emulated_kernels import aligned, emu  # noqa: F401  (the x86 emulator build of the same sources)

N = 16
ERR_NULL, ERR_LAYERS, ERR_PRECISION, ERR_WORKSPACE, ERR_SIZE = -1, -2, -3, -4, -5
# the smallest net of each family, one with a wrong output count for it, and the other family's input count
NETS = {"wave": ([3, 32, 32, 7], [3, 32, 32, 5], [4, 32, 32, 7]),
        "plate": ([3, 32, 32, 5], [3, 32, 32, 7], [4, 32, 32, 5]),
        "nc3d": ([4, 32, 32, 12], [4, 32, 32, 7], [3, 32, 32, 12])}

# argument names of the entry points, in the segments capi.PROTOTYPES is written in
NET = ("params", "layers", "n_layers")
PTS3 = ("x", "y", "t", "n", "lb", "ub", "normalize")
PTS4 = ("x", "y", "z", "t", "n", "lb", "ub", "normalize")
MAT = ("E", "mu", "rho")
WAVE = MAT + ("plane_strain", "term_weights")
OUT = ("loss_terms_out", "grad_flat_out", "accumulate")
TAIL = ("precision_mode", "workspace", "ws_bytes", "stream")
SUMS = ("sums_out",) + TAIL[:3] + ("sums_workspace", "sums_ws_bytes", "stream")
ENTRIES = {      # symbol -> (family, argument names)
    "pinn_wave2d_loss_grad": ("wave", NET + PTS3 + WAVE + OUT + TAIL),
    "pinn_data_loss_grad": ("wave", NET + PTS3 + ("targets", "out_weights") + OUT + TAIL),
    "pinn_wave2d_fields": ("wave", NET + PTS3 + ("fields_out",) + TAIL),
    "pinn_wave2d_residual_score": ("wave", NET + PTS3 + WAVE + ("score_out",) + TAIL),
    "pinn_wave2d_predict": ("wave", NET + PTS3 + ("out",) + TAIL),
    "pinn_wave2d_material_sums": ("wave", NET + PTS3 + MAT + ("plane_strain",) + SUMS),
    "pinn_net_streams": ("plate", NET + PTS3 + ("streams_out",) + TAIL),
    "pinn_plate2d_loss_grad": ("plate", NET + PTS3 + ("frozen_streams",) + MAT + ("term_weights",) + OUT + TAIL),
    "pinn_plate2d_residual_score": ("plate", NET + PTS3 + ("frozen_streams",) + MAT + ("term_weights", "score_out") + TAIL),
    "pinn_plate2d_material_sums": ("plate", NET + PTS3 + ("frozen_streams",) + MAT + SUMS),
    "pinn_plate2d_predict": ("plate", NET + PTS3 + ("frozen_streams", "out") + TAIL),
    "pinn_plate2d_traction_loss_grad": ("plate", NET + PTS3 + ("frozen_and_normals", "weights") + OUT + TAIL),
    "pinn_stream_loss_grad": ("plate", NET + PTS3 + ("targets", "weights") + OUT + TAIL),
    "pinn_nc3d_loss_grad": ("nc3d", NET + PTS4 + MAT + ("term_weights",) + OUT + TAIL),
    "pinn_nc3d_data_loss_grad": ("nc3d", NET + PTS4 + ("targets", "out_weights") + OUT + TAIL),
    "pinn_nc3d_fields": ("nc3d", NET + PTS4 + ("fields_out",) + TAIL),
    "pinn_nc3d_residual_score": ("nc3d", NET + PTS4 + MAT + ("term_weights", "score_out") + TAIL),
    "pinn_nc3d_material_sums": ("nc3d", NET + PTS4 + MAT + SUMS),
}
COLUMNS = ("x", "y", "z", "t")
# pointers every entry point hands to prepare(); every other pointer argument is the entry's own
COMMON = ("params", "layers", "lb", "ub", "workspace", "stream") + COLUMNS
OUTPUTS = ("loss_terms_out", "fields_out", "score_out", "out", "sums_out", "streams_out")
SCALARS = {"n": N, "normalize": 1, "E": 2.5, "mu": 0.25, "rho": 1.0, "plane_strain": 1, "accumulate": 0, "precision_mode": PREC["f16x3"]}


def is_pointer(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def own_pointers(symbol):
    names = ENTRIES[symbol][1]
    return [a for a, t in zip(names, PROTOTYPES[symbol][1]) if is_pointer(t) and a not in COMMON]


class Memory:
    """the buffers of the valid calls, shared by every entry point of one library and kept alive by the sweep"""

    def __init__(self, lib):
        rng = np.random.default_rng(7)
        nets = [net for family in NETS.values() for net in family]
        self.ws_bytes = max(lib.workspace_bytes(net, 4096, "f16x3") for net in nets)
        self.sums_ws_bytes = lib.material_sums_workspace_bytes()
        self.bufs = {"workspace": aligned(self.ws_bytes), "sums_workspace": aligned(self.sums_ws_bytes + 256),
                     "params": aligned(1 << 16).view(np.float32), "lb": np.zeros(4), "ub": np.ones(4)}
        self.bufs["params"][:] = 0.1 * rng.standard_normal(self.bufs["params"].size)
        for col in COLUMNS:
            self.bufs[col] = rng.random(N).astype(np.float32)
        self.ones = np.ones(64, dtype=np.float32)      # every weight argument (term_weights[<= 12], out_weights[<= 16], weights[5][<= 8])

    def valid(self, symbol):
        """argument name -> value of a call of `symbol` with which nothing is wrong"""
        family, names = ENTRIES[symbol]
        argtypes = PROTOTYPES[symbol][1]
        assert len(names) == len(argtypes), symbol
        args = {}
        for a, t in zip(names, argtypes):
            if a == "layers":
                args[a] = NETS[family][0]
            elif a == "n_layers":
                args[a] = None      # (follows `layers`)
            elif a == "stream":
                args[a] = None
            elif a in ("ws_bytes", "sums_ws_bytes"):
                args[a] = getattr(self, a)
            elif not is_pointer(t):
                args[a] = SCALARS[a]
            elif t is C.c_void_p:
                if a not in self.bufs:
                    self.bufs[a] = aligned(1 << 16)      # an output, the frozen streams, the targets: zeros, larger than any head reads or writes
                args[a] = self.bufs[a].ctypes.data
            else:
                args[a] = (self.ones if t._type_ is C.c_float else self.bufs[a]).ctypes.data_as(t)
        return args


def cases(symbol):
    """(case, {argument: value in place of the valid one, or a function of the valid one}) in the order they are recorded in"""
    family, names = ENTRIES[symbol]
    _, wrong_nout, wrong_din = NETS[family]
    out = next(a for a in names if a in OUTPUTS)
    short = {"sums_ws_bytes": lambda nbytes: nbytes - 1}
    yield "valid", {}
    for a in ["params", "workspace"] + [c for c in COLUMNS if c in names] + own_pointers(symbol):
        yield f"{a} NULL", {a: None}
    yield "n = -1", {"n": -1}
    yield "normalize, lb NULL", {"lb": None}
    yield "precision 7", {"precision_mode": 7}
    if family != "wave":      # the five-stream and four-input kernels exist for the split modes only
        yield "bf16", {"precision_mode": PREC["bf16"]}
        yield "f16", {"precision_mode": PREC["f16"]}
    yield "layers [3, 32, 48, 7]", {"layers": [3, 32, 48, 7]}
    yield "wrong output count", {"layers": wrong_nout}
    yield "wrong input count", {"layers": wrong_din}
    if "sums_workspace" in names:
        yield "sums workspace off alignment", {"sums_workspace": lambda address: address + 8}
        yield "sums workspace one byte short", short
    yield "n = -1, params NULL", {"n": -1, "params": None}
    yield f"{out} NULL, wrong output count", {out: None, "layers": wrong_nout}
    if "sums_workspace" in names:
        yield "wrong output count, sums workspace one byte short", {"layers": wrong_nout, **short}


def call(lib, symbol, args):
    """the raw entry point: the integer code, no exception"""
    args = dict(args)
    layers = args["layers"]
    args["layers"], args["n_layers"] = lib._ints(layers), len(layers)
    return int(getattr(lib.lib, symbol)(*[args[a] for a in ENTRIES[symbol][1]]))


def sweep(lib, only=None):
    """symbol -> {case: return code}; `only(symbol, case)` picks the cases to run"""
    lib.set_fused(1)
    mem = Memory(lib)
    table = {}
    for symbol in ENTRIES:
        valid = mem.valid(symbol)
        table[symbol] = {}
        for case, change in cases(symbol):
            if only is None or only(symbol, case):
                change = {a: v(valid[a]) if callable(v) else v for a, v in change.items()}
                table[symbol][case] = call(lib, symbol, {**valid, **change})
    return table


def differences(expected, got):
    return {(symbol, case): (expected[symbol][case], got[symbol][case]) for symbol in got for case in got[symbol]
            if expected[symbol][case] != got[symbol][case]}


def test_every_entry_point_is_swept():
    assert set(ENTRIES) == set(parent.CODES) and set(ENTRIES) <= set(PROTOTYPES) and len(ENTRIES) == 18
    for symbol in ENTRIES:
        assert [case for case, _ in cases(symbol)] == list(parent.CODES[symbol]), symbol      # (a case added later needs its recorded code)


def test_argument_errors_answer_as_before_emulator_build(emu):
    got = sweep(emu)
    bad = differences(parent.CODES, got)
    assert not bad, f"return code moved for {len(bad)} cases ((entry, case): (before, now)): {bad}"
    assert sum(len(v) for v in got.values()) == sum(len(v) for v in parent.CODES.values())


def test_argument_errors_answer_as_before_gfx950_build(lib):
    got = sweep(lib, only=lambda symbol, case: parent.CODES[symbol][case] < 0)
    bad = differences(parent.CODES, got)
    assert not bad, f"return code moved for {len(bad)} cases ((entry, case): (before, now)): {bad}"
    assert sum(len(v) for v in got.values()) == sum(code < 0 for v in parent.CODES.values() for code in v.values())


def test_the_sweep_reaches_every_answer():
    """the recorded table holds every code the checks can give and the valid call of every entry point; a sweep that records one code
    would prove nothing"""
    codes = {code for v in parent.CODES.values() for code in v.values()}
    assert {0, ERR_NULL, ERR_LAYERS, ERR_PRECISION, ERR_WORKSPACE, ERR_SIZE} <= codes, codes
    assert all(v["valid"] == 0 for v in parent.CODES.values())
    # the precedence the pairs pin: a NULL params before a negative n, a NULL output before the output count, the output count before the sums workspace
    for symbol, v in parent.CODES.items():
        assert v["n = -1"] == ERR_SIZE and v["n = -1, params NULL"] == ERR_NULL, symbol
        if "wrong output count, sums workspace one byte short" in v:
            assert v["sums workspace one byte short"] == ERR_WORKSPACE and v["wrong output count, sums workspace one byte short"] == ERR_LAYERS, symbol
