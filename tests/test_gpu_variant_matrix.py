"""-m gpu: the variant matrix (tests/_variant_matrix.py) on the device -- every row at the six sizes around the 16-point tile and the
workgroup step with every entry point of its head, the fused rows also at the full-grid edges 256 * 16 * TILES * k + {-1, 0, +1}
(k = 1, 3: the last step partial on a full 256-workgroup grid, the XCD-aware tail), and the narrow fused kernels' precision statement of
include/pinn_hip.h (PINN_PREC_BF16X3) at 64 / 1024 / 16384 points."""
import numpy as np
import pytest
import torch

from tests import _variant_matrix as vm

pytestmark = pytest.mark.gpu

# the eight-layer instantiations of the register layouts (a different state-parking plan than the four-layer ones)
GPU_ROWS = vm.ROWS + (vm.R("f16x3", 50, 8, "wave data plate", "fused-registers") + vm.R("bf16x3", 50, 8, "wave data plate", "fused-registers")
                      + vm.R("bf16", 50, 8, "wave data", "fused-registers") + vm.R("f16", 50, 8, "wave data", "fused-registers"))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("row", GPU_ROWS, ids=str)
def test_variant_matrix_gpu(lib, dev, row):
    for n in row.sizes:
        vm.check_row(lib, vm.Mem(dev), row, n)
    vm.check_empty(lib, vm.Mem(dev), row)


EDGE_ROWS = [r for r in GPU_ROWS if r.path.startswith("fused")]


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("row", EDGE_ROWS, ids=str)
def test_variant_matrix_full_grid_edges_gpu(lib, dev, row, k):
    full = 256 * 16 * row.tiles * k
    for n in (full - 1, full, full + 1):
        vm.check_row(lib, vm.Mem(dev), row, n, full=False)


@pytest.mark.parametrize("row", [r for r in GPU_ROWS if r.path.startswith("fused") or (r.path == "two-kernel" and r.width <= 64)], ids=str)
def test_variant_matrix_walks_gpu(lib, dev, row):
    """every fused layout with its grid capped at 64 workgroups (the fewest a persistent launch takes, FUSED_MIN_GRID) over
    2 * 64 * 16 * TILES + 5 points -- three steps for some workgroups, the last one partial --, and every layout of padded width <= 64 with
    pinn_min_workspace_bytes (chunked passes, or the two-kernel path where the minimum holds too few scratch images)"""
    if row.path.startswith("fused"):
        vm.check_walk(lib, vm.Mem(dev), row, 2 * 64 * 16 * row.tiles + 5, grid_cap=64)
    if row.width <= 64:
        vm.check_walk(lib, vm.Mem(dev), row, 20000, min_ws=True)      # (more steps than the minimum holds images: the path pinn_path_for names)


@pytest.mark.parametrize("row", [r for r in GPU_ROWS if r.path == "fused-registers" and r.prec == "bf16x3"], ids=str)
def test_bf16x3_narrow_precision_statement(lib, dev, row):
    """include/pinn_hip.h, PINN_PREC_BF16X3: the narrow fused kernels take the layer states as bf16 high parts in the weight gradient --
    an error that falls as c / sqrt(points) (tools/narrow_noise_study.py measures c).  Held at 64 / 1024 / 16384 points with the matrix's
    bar and the two-kernel path (both parts of both factors) at the mode's bar; and it does fall: 256 times the points, at least 4 times
    less error (16 by the statement)."""
    err = {n: vm.check_row(lib, vm.Mem(dev), row, n, full=False) for n in (64, 1024, 16384)}
    assert err[16384] < err[64] / 4, (str(row), err)
