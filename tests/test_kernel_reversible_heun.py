"""The reversible Heun kernels stay out of scratch (no GPU needed): csrc/revheun.hip is compiled for gfx950 with the project's
own flags and the compiler's resource report is read, as tests/test_kernel_resources.py does for the default path.  The
backward kernel carries five state vectors beside the 128 dL/dW accumulators at one wave per SIMD; a few more live registers
and the compiler answers with scratch traffic in every node."""
import pytest

from torchcde_amd import _lib
from test_kernel_resources import _resources

SRC = "revheun.hip"


@pytest.fixture(scope="module")
def report():
    assert SRC in _lib.SOURCES
    return _resources(SRC)


@pytest.mark.parametrize("kernel,instantiations", [
    ("revheun_forward_mfma<", 8),      # f32 / f64 time x cubic / linear x identity / tanh
    ("revheun_adjoint_mfma<", 8),
])
def test_reversible_heun_kernels_use_no_scratch(report, kernel, instantiations):
    found = {n: r for n, r in report.items() if kernel in n}
    assert len(found) == instantiations, sorted(found)
    spilled = {n: (r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for n, r in found.items()
               if r.get("ScratchSize [bytes/lane]") != "0" or r.get("VGPRs Spill") != "0"}
    assert not spilled, "scratch (bytes per lane, spilled VGPRs): %s" % spilled
    if "forward" in kernel:                   # two waves per SIMD need <= 256 registers
        assert all(int(r["VGPRs"]) + int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found
    else:                                     # one wave per SIMD: the whole register file, and no more
        assert all(int(r["VGPRs"]) <= 256 and int(r.get("AGPRs", "0")) <= 256 for r in found.values()), found
