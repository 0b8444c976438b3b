"""The broad-inner-layer kernels of the two-layer field stay out of scratch (no GPU needed): csrc/rk4_mlp_broad.hip is compiled
for gfx950 with the project's own flags and the compiler's resource report is read, as tests/test_kernel_mlp_tiled.py does.
The forward kernel (K2mb) claims two waves per SIMD (512-thread bounds: at most 256 registers), the sweep (K3mb) one
(256-thread bounds: u and gu of 64 registers each, two operand sets and the RK state of z and a need more than 256)."""
import pytest

from torchcde_amd import _lib
from test_kernel_resources import _resources

SRC = "rk4_mlp_broad.hip"


@pytest.fixture(scope="module")
def report():
    assert SRC in _lib.SOURCES
    return _resources(SRC)


@pytest.mark.parametrize("kernel,instantiations", [
    ("rk4_forward_mlp_broad<", 32),          # f32 / f64 time x cubic / linear x (identity / tanh) x (relu / softplus) x VEC
    ("rk4_adjoint_mlp_broad_sweep<", 16),    # the same without VEC: the sweep reads padded copies
])
def test_broad_kernels_use_no_scratch(report, kernel, instantiations):
    found = {n: r for n, r in report.items() if kernel in n}
    assert len(found) == instantiations, sorted(found)
    spilled = {n: (r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for n, r in found.items()
               if r.get("ScratchSize [bytes/lane]") != "0" or r.get("VGPRs Spill") != "0"}
    assert not spilled, "scratch (bytes per lane, spilled VGPRs): %s" % spilled
    if "forward" in kernel:                   # two waves per SIMD need <= 256 registers
        assert all(int(r["VGPRs"]) + int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found
        assert all(r.get("Occupancy [waves/SIMD]") == "2" for r in found.values()), found
    else:                                     # one wave per SIMD: the whole register file, and no more
        assert all(int(r["VGPRs"]) <= 256 and int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found
        assert all(r.get("Occupancy [waves/SIMD]") == "1" for r in found.values()), found


def test_the_image_kernel_is_the_only_other_kernel_of_the_file(report):
    """One more kernel builds the sweep's images; nothing of the file uses scratch, and none of its kernels carries "tiled" in
    its name (tests/test_kernel_mlp_tiled.py counts those in its own file)."""
    assert sum("mlp_broad_adj_image_kernel" in n for n in report) == 1
    own = {n: r for n, r in report.items() if "broad" in n}
    assert len(own) == 32 + 16 + 1, sorted(own)
    assert all(r.get("ScratchSize [bytes/lane]") == "0" for r in own.values()), own
    assert not any("tiled" in n for n in report), sorted(report)
