"""The wide-control kernels of the two-layer field stay out of scratch (no GPU needed): csrc/rk4_mlp_widec.hip is compiled for
gfx950 with the project's own flags and the compiler's resource report is read, as tests/test_kernel_reversible_heun.py does.
The forward kernel claims two waves per SIMD (512-thread bounds), the sweep one (256-thread bounds: under the forward kernel's
bounds it spilled 164 bytes per lane)."""
import pytest

from torchcde_amd import _lib
from test_kernel_resources import _resources

SRC = "rk4_mlp_widec.hip"


@pytest.fixture(scope="module")
def report():
    assert SRC in _lib.SOURCES
    return _resources(SRC)


@pytest.mark.parametrize("kernel,instantiations", [
    ("rk4_forward_mlp_widec<", 32),          # f32 / f64 time x cubic / linear x (identity / tanh) x (relu / softplus) x VEC
    ("rk4_adjoint_mlp_widec_sweep<", 16),    # the same without VEC: the sweep reads padded copies
])
def test_wide_control_kernels_use_no_scratch(report, kernel, instantiations):
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
