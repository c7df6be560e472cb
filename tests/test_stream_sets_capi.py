"""CPU tests of pinn_stream_loss_grad_multi's host side: the symbol, the binding's struct, and what pinn_path_for answers for the new
head.  No device work."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST = [3, 20, 20, 20, 20, 5]          # the reference's distance / particular nets (PLATE:527-559)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib()


def w(depth, width, nout=5):
    return [3] + depth * [width] + [nout]


def test_symbol_is_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    assert re.search(r"\bint\s+pinn_stream_loss_grad_multi\s*\(", src)
    assert re.search(r"#define\s+PINN_MAX_STREAM_SETS\s+8\b", src) and re.search(r"PINN_HEAD_STREAM_SETS\s*=\s*6\b", src)
    assert hasattr(lib.lib, "pinn_stream_loss_grad_multi")
    assert lib.abi_version() == 2           # additive


def test_binding_struct_matches_the_header():
    from pinn_elastodynamics_amd.capi import HEADS, MAX_STREAM_SETS, StreamSet
    assert HEADS["stream_sets"] == 6 and MAX_STREAM_SETS == 8
    # x, y, t (3 pointers), n (int64), targets (pointer), weights[5][8] floats, loss_terms_out (pointer)
    assert ctypes.sizeof(StreamSet) == 5 * 8 + 160 + 8
    assert StreamSet.weights.offset == 40 and StreamSet.loss_terms_out.offset == 200


def test_kernel_is_in_the_shared_object(lib):
    blob = open(os.path.join(ROOT, "pinn_elastodynamics_amd", "lib", "libpinn_hip.so"), "rb").read()
    assert b"fused_sets_kernel" in blob and b"reduce_grad_loss_sets_kernel" in blob


def test_path_for_stream_sets(lib):
    from pinn_elastodynamics_amd.capi import FLAG_TWO_KERNEL, PREC, PinnLibError
    assert lib.path_for(DIST, "f16x3", "stream_sets") == "fused-registers"
    assert lib.path_for(w(4, 50), "f16x3", "stream_sets") == "fused-registers"
    assert lib.path_for(w(4, 50), "bf16x3", "stream_sets") == "fused-registers"          # (bf16x3 is compiled at padded width 64)
    for layers in (w(3, 20), w(5, 20), w(8, 20), w(4, 70)):
        assert lib.path_for(layers, "f16x3", "stream_sets") == "two-kernel", layers
    assert lib.path_for(DIST, PREC["f16x3"] | FLAG_TWO_KERNEL, "stream_sets") == "two-kernel"
    assert lib.path_for(DIST, "f16x3", "stream_sets", lib.min_workspace_bytes(DIST, "f16x3") // 2) == "two-kernel"
    assert lib.path_for(DIST, "fp32", "stream_sets") == "fp32"
    with pytest.raises(PinnLibError):
        lib.path_for(DIST, "bf16", "stream_sets")
    # the one-set call keeps its path
    assert lib.path_for(DIST, "f16x3", "streams") == "two-kernel"


def test_path_for_honours_the_workspace(lib):
    """The workspace of the largest set is enough at the reference's set sizes (examples/plate_hole.py: DIST 45 000 points, the boundary sets
    251 x 101 and 101 x 101 points); a workspace that holds fewer than 64 scratch images is reported as what it gives."""
    for n_max in (45000, 251 * 101, 101 * 101, 3000):
        assert lib.path_for(DIST, "f16x3", "stream_sets", lib.workspace_bytes(DIST, n_max, "f16x3")) == "fused-registers", n_max
        assert lib.path_for(w(4, 50), "f16x3", "stream_sets", lib.workspace_bytes(w(4, 50), n_max, "f16x3")) == "fused-registers", n_max
    assert lib.path_for(DIST, "f16x3", "stream_sets", lib.workspace_bytes(DIST, 64, "f16x3")) == "two-kernel"


def test_argument_errors_need_no_device(lib):
    from pinn_elastodynamics_amd.capi import PinnLibError
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ws = (p + 255) // 256 * 256
    row = (p, p, p, 4, 0, [[1.0] * 5] * 5, p)
    with pytest.raises(PinnLibError, match="NULL"):
        lib.stream_loss_grad_multi(p, DIST, [row], [0, 0, 0], [1, 1, 1], False, 0, False, "f16x3", ws, 64)          # no gradient buffer
    with pytest.raises(PinnLibError, match="NULL"):
        lib.stream_loss_grad_multi(p, DIST, [(0, p, p, 4, 0, row[5], p)], [0, 0, 0], [1, 1, 1], False, p, False, "f16x3", ws, 64)
    with pytest.raises(PinnLibError, match="negative"):
        lib.stream_loss_grad_multi(p, DIST, [(p, p, p, -1, 0, row[5], p)], [0, 0, 0], [1, 1, 1], False, p, False, "f16x3", ws, 64)
    with pytest.raises(PinnLibError, match="precision"):
        lib.stream_loss_grad_multi(p, DIST, [row], [0, 0, 0], [1, 1, 1], False, p, False, "bf16", ws, 64)
