"""The tiled kernels of the one-layer field on wide controls stay out of scratch (no GPU needed): csrc/rk4_affine_tiled.hip is
compiled for gfx950 with the project's own flags and the compiler's resource report is read, as tests/test_kernel_mlp_tiled.py
does for the two-layer field.  The forward kernel K2c claims at least two waves per SIMD (512-thread bounds: at most 256
registers; without a first layer's operands it fits four), the sweep K3c at least one (256-thread bounds, as K3mc)."""
import pytest

from torchcde_amd import _lib
from test_kernel_resources import _resources

SRC = "rk4_affine_tiled.hip"


@pytest.fixture(scope="module")
def report():
    assert SRC in _lib.SOURCES
    return _resources(SRC)


@pytest.mark.parametrize("kernel,instantiations", [
    ("rk4_forward_affine_tiled<", 16),         # f32 / f64 time x cubic / linear x identity / tanh x VEC
    ("rk4_adjoint_affine_tiled_sweep<", 8),    # the same without VEC: the sweep reads a padded image
])
def test_tiled_kernels_use_no_scratch(report, kernel, instantiations):
    found = {n: r for n, r in report.items() if kernel in n}
    assert len(found) == instantiations, sorted(found)
    spilled = {n: (r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for n, r in found.items()
               if r.get("ScratchSize [bytes/lane]") != "0" or r.get("VGPRs Spill") != "0"}
    assert not spilled, "scratch (bytes per lane, spilled VGPRs): %s" % spilled
    if "forward" in kernel:                    # two waves per SIMD (or more) need <= 256 registers
        assert all(int(r["VGPRs"]) + int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found
        assert all(int(r.get("Occupancy [waves/SIMD]")) >= 2 for r in found.values()), found
    else:                                      # one wave per SIMD: the whole register file, and no more
        assert all(int(r["VGPRs"]) <= 256 and int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found


def test_the_small_kernels_of_the_file_use_no_scratch(report):
    """The image, seed and gather kernels are the only other kernels of the file."""
    small = {n: r for n, r in report.items() if n.startswith("cde::affine_tiled_") or n.startswith("affine_tiled_")}
    assert len(small) == 3, sorted(report)
    assert all(r.get("ScratchSize [bytes/lane]") == "0" for r in small.values()), small
    assert sum("affine_tiled" in n for n in report) == 16 + 8 + 3, sorted(report)
