"""CPU, host calls only (no kernel launch): the decisions of the host dispatch -- which net takes which fused instantiation, and how many
scratch images a workspace must hold for it -- pinned for every compiled line x head x depth x workspace size.  The expected answers
(tests/_dispatch_parent.py) were recorded from the build before Host::with_fused single-sourced those decisions and are not regenerated:
pinn_path_for must answer as it did for every input, and pinn_debug_cache_policy must reproduce every answer it gave.

The material constants of the plate and 3-D entry points (the Hooke coefficients now all come from one function) are held at
non-degenerate values by tests/test_emulated_constants.py: test_plate_head_general_constants_emulated (E 7.3 / nu 0.31 / rho 1.7, every
path, per term) and test_nc3d_head_general_constants_emulated (sets A and B)."""
import ctypes as C

from pinn_elastodynamics_amd.capi import HEADS, PREC
from tests import _dispatch_parent as parent
from tests._variant_matrix import PREC_OF, variant_lines
from tests.test_capi_symbols import lib  # noqa: F401  (the gfx950 library: its host-only entry points run without a GPU)
from tests.test_emulated_kernels import emu  # noqa: F401  (the x86 emulator build of the same sources)

DEPTHS = (2, 4, 6, 8, 10)
# the head's natural (outputs, inputs)
SHAPE = {"wave": (7, 3), "data": (7, 3), "plate": (5, 3), "nc3d": (12, 4), "nc3d_data": (12, 4), "streams": (5, 3), "stream_sets": (5, 3)}
WS_CASES = ("0", "min // 2", "min", "n = 4096", "n = 1 << 20")
ERR_LAYERS = -2
CODE = {1: "1", 2: "2", 3: "3", -2: "L", -3: "P"}      # the characters of tests/_dispatch_parent.py


def net(head, depth, width):
    nout, din = SHAPE[head]
    return [din] + depth * [width] + [nout]


def ws_sizes(lib, layers, prec):
    mn = lib.min_workspace_bytes(layers, prec)
    return (0, mn // 2, mn, lib.workspace_bytes(layers, 4096, prec), lib.workspace_bytes(layers, 1 << 20, prec))


def raw_path_for(lib, layers, prec, head, ws_bytes):
    return int(lib.lib.pinn_path_for(lib._ints(layers), len(layers), PREC[prec], HEADS[head], int(ws_bytes)))


def path_sweep(lib):
    """'<line> <head>' -> pinn_path_for over DEPTHS x WS_CASES, in the notation of tests/_dispatch_parent.py"""
    out = {}
    for op, split, width in variant_lines():
        prec = PREC_OF[(op, split)]
        for head in HEADS:
            out[f"{op}_{split}_{width} {head}"] = " ".join(
                "".join(CODE[raw_path_for(lib, net(head, depth, width), prec, head, ws)] for ws in ws_sizes(lib, net(head, depth, width), prec))
                for depth in DEPTHS)
    return out


def raw_cache_policy(lib, layers, head):
    im, su = C.c_size_t(0), C.c_size_t(0)
    fn = lib.lib.pinn_debug_cache_policy
    fn.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    fn.restype = C.c_int
    rc = int(fn(lib._ints(layers), len(layers), HEADS[head], C.byref(im), C.byref(su)))
    return rc if rc < 0 else (rc, int(im.value), int(su.value))


def cache_sweep(lib):
    widths = sorted({w for _, _, w in variant_lines()})
    return {(head, width): {depth: raw_cache_policy(lib, net(head, depth, width), head) for depth in DEPTHS}
            for head in ("wave", "plate", "nc3d") for width in widths}


def check_paths(lib, expected):
    got = path_sweep(lib)
    assert got.keys() == expected.keys()          # (a new line of pinn_variants.def needs its rows)
    bad = {key: (expected[key], got[key]) for key in expected if expected[key] != got[key]}
    assert not bad, f"pinn_path_for moved for {len(bad)} rows (line head: before, now; depths {DEPTHS} x workspaces {WS_CASES}): {bad}"


def test_path_for_answers_as_before_gfx950_build(lib):
    check_paths(lib, parent.PATHS_HIP)


def test_path_for_answers_as_before_emulator_build(emu):
    check_paths(emu, parent.PATHS_EMU)


def test_the_sweep_reaches_every_answer():
    """the recorded table holds every path and both errors, and the two builds differ only where the minimum grid (64 / 1) decides"""
    for tab in (parent.PATHS_HIP, parent.PATHS_EMU):
        assert set("".join(tab.values())) == set("123P ")
    differ = {(key, i) for key in parent.PATHS_HIP for i in range(29) if parent.PATHS_HIP[key][i] != parent.PATHS_EMU[key][i]}
    assert differ and all(i % 6 in (1, 2) and parent.PATHS_HIP[key][i] == "3" for key, i in differ), sorted(differ)


def check_cache_policy(lib):
    got = cache_sweep(lib)
    assert got.keys() == parent.CACHE_POLICY.keys()
    newly = []
    for (head, width), rows in parent.CACHE_POLICY.items():
        for depth, before in rows.items():
            now = got[(head, width)][depth]
            if before != ERR_LAYERS:
                assert now == before, (head, width, depth, before, now)
                continue
            fused = raw_path_for(lib, net(head, depth, width), "f16x3", head, 0) in (1, 2)
            if not fused:
                assert now == ERR_LAYERS, (head, width, depth, now)
            elif now != ERR_LAYERS:        # a compiled layout the hand-written list had forgotten
                policy, images, sums = now
                assert policy in (0, 1, 2) and images > 0 and sums > 0, (head, width, depth, now)
                newly.append((head, width, depth))
    return newly


def test_cache_policy_answers_as_before_gfx950_build(lib):
    check_cache_policy(lib)


def test_cache_policy_answers_as_before_emulator_build(emu):
    check_cache_policy(emu)
