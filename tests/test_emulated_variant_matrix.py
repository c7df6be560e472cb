"""CPU half of the variant matrix (tests/_variant_matrix.py): every line of pinn_variants.def x every head pinn_path_for admits for it, on
the host SIMT emulator, against the float64 oracle -- sizes around the 16-point tile and the workgroup step, guard words behind every
output, accumulate / overwrite / empty batch, the packed-weights flag, the same call off the fused kernel.  And the completeness test:
a variant line, an admitted head or a path without a row fails it."""
import os
import subprocess

import pytest

from tests import _variant_matrix as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["make", "-C", os.path.join(ROOT, "pinn_elastodynamics_amd", "csrc"), "-j", str(min(16, os.cpu_count() or 1)), "emu"],
                   check=True, capture_output=True)
    from pinn_elastodynamics_amd.capi import PinnLib
    return PinnLib(os.path.join(ROOT, "build", "emu", "libpinn_emu.so"))


def test_matrix_is_complete(emu):
    """Every PINN_VARIANT line maps to a precision mode and has rows; every head pinn_path_for admits for a line (at any real width and
    depth the generator tries) has a row of that line; every path pinn_path_for names for the generated cases is exercised by a row.
    Host-only: no kernel runs."""
    lines = vm.variant_lines()
    assert len(lines) == len(set(lines)) and lines, lines
    covered = {(r.line, r.head) for r in vm.ROWS}
    missing, named = [], set()
    for line, head, layers in vm.generated_cases(lines):
        assert line == vm.FP32_LINE or vm.prec_of(line), f"{line}: no precision mode for this operand type / split"
        assert layers is not None, f"{line}: no real hidden widths for padded width {line[2]}"
        try:
            path = emu.path_for(layers, vm.prec_of(line), head)
        except Exception:
            continue
        named.add(path)
        if (line, head) not in covered:
            missing.append((line, head))
    assert not missing, f"admitted (variant line, head) pairs without a row in tests/_variant_matrix.py: {sorted(set(missing))}"
    assert named <= {r.path for r in vm.ROWS}, named
    row_lines = {r.line for r in vm.ROWS}
    assert set(lines) | {vm.FP32_LINE} <= row_lines, f"variant lines without a row: {sorted(set(lines) - row_lines)}"
    assert row_lines <= set(lines) | {vm.FP32_LINE}, f"rows of a line that is not in pinn_variants.def: {sorted(row_lines - set(lines))}"
    for r in vm.ROWS:                  # each row lands where it says
        assert emu.path_for(r.layers, r.prec, r.head) == r.path, str(r)


# What the emulator runs of each row (the GPU half runs every row at all six sizes with every entry point).  Emulated cost grows with the
# padded width and the streams: one 16-point step of the 10 x 128 3-D kernel takes ~3 s, of the 4 x 20 register layout ~0.05 s.  So:
#   - every row of padded width <= 64, every fp32 row and every bf16 row (the lines of padded width 96 / 128 / 160 without a fused
#     instantiation): the primary entry point at all six sizes, every other entry point and check at n = 17;
#   - the one-stream LDS-operand layouts (data head at 96 / 128 / 160) and the four-stream one at 96: all six sizes (primary entry point,
#     the same call under PINN_FLAG_TWO_KERNEL at n = 17); the five-stream one at 96 (plate): n = 17 and 16 * TILES + 1;
#   - the f16x3 two-kernel rows of padded width 96 / 128 / 160 (plate / streams / 4-input heads): n = 1, and every entry point at n = 17;
#   - GPU only: the wide four-stream layouts at 128 / 160 and the 3-D five-stream layout (tests/test_emulated_kernels.py holds them at
#     ragged sizes: test_fused_wide_emulated, test_fused_width160_emulated, test_fused_nc3d_emulated) and the other entry points of the
#     LDS-operand rows.
GPU_ONLY = {"f16x3-8x100-wave-fused-lds", "f16x3-6x140-wave-fused-lds", "f16x3-10x100-nc3d-fused-lds"}


def emu_plan(row):
    """(sizes of the primary entry point, size of the check of every entry point or None)"""
    if row.width <= 64 or row.prec in ("fp32", "bf16"):
        return [n for n in row.sizes if n != 17], 17
    if row.path == "fused-lds":
        sizes = row.sizes if row.head in ("data", "nc3d_data", "wave") else (17, 16 * row.tiles + 1)
        return list(sizes), None
    return [1], 17


@pytest.mark.parametrize("row", [r for r in vm.ROWS if str(r) not in GPU_ONLY], ids=str)
def test_variant_matrix_emulated(emu, row):
    sizes, full = emu_plan(row)
    for n in sizes:
        vm.check_row(emu, vm.Mem(), row, n, full=False, two_kernel=(n == 17))
    if full:
        vm.check_row(emu, vm.Mem(), row, full)
    vm.check_empty(emu, vm.Mem(), row)


# one capped-grid walk per fused layout family of the emulator half (register layouts: four-, five- and one-stream; LDS-operand: one-stream)
# and two minimum-workspace runs that really chunk (2100 points against the minimum's 64 tiles of 32: two passes; the GPU half walks every
# layout of padded width <= 64 this way)
CHUNKED = {"f16x3-4x20-wave-fused-registers", "f16x3-2x20-streams-two-kernel"}
WALK_ROWS = [r for r in vm.ROWS if (r.path == "fused-registers" and r.prec == "f16x3") or str(r) in CHUNKED or str(r) == "f16x3-8x70-data-fused-lds"]


@pytest.mark.parametrize("row", WALK_ROWS, ids=str)
def test_variant_matrix_walks_emulated(emu, row):
    """A fused grid capped at 3 workgroups over 2 * 3 * 16 * TILES + 5 points (three steps for some workgroups, the last one partial);
    the minimum workspace (the call walks the points in chunks, or leaves the fused kernel)."""
    if row.path.startswith("fused"):
        vm.check_walk(emu, vm.Mem(), row, 2 * 3 * 16 * row.tiles + 5, grid_cap=3)
    if str(row) in CHUNKED:
        vm.check_walk(emu, vm.Mem(), row, 2100, min_ws=True)
