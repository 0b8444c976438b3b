"""The tiled-output-layer kernels of the two-layer field stay out of scratch (no GPU needed): csrc/rk4_mlp_tiled.hip is compiled
for gfx950 with the project's own flags and the compiler's resource report is read, as tests/test_kernel_reversible_heun.py
does.  One source, two forms told apart by the first template argument NV, the state vectors a lane owns: 2 = wide control
(K2mc / K3mc), 4 = tall state (K2mh / K3mh).  The forward kernel claims two waves per SIMD (512-thread bounds: at most 256
registers), the sweep one (256-thread bounds: under the forward kernel's bounds NV = 2 spilled 164 bytes per lane, and the
doubled state of NV = 4 -- z and a, their RK temporaries, u, gu and two operand sets -- needs more than 256)."""
import pytest

from torchcde_amd import _lib
from test_kernel_resources import _resources

SRC = "rk4_mlp_tiled.hip"
FORMS = [2, 4]


@pytest.fixture(scope="module")
def report():
    assert SRC in _lib.SOURCES
    return _resources(SRC)


@pytest.mark.parametrize("nv", FORMS)
@pytest.mark.parametrize("kernel,instantiations", [
    ("rk4_forward_mlp_tiled<", 32),          # f32 / f64 time x cubic / linear x (identity / tanh) x (relu / softplus) x VEC
    ("rk4_adjoint_mlp_tiled_sweep<", 16),    # the same without VEC: the sweep reads padded copies
])
def test_tiled_kernels_use_no_scratch(report, nv, kernel, instantiations):
    found = {n: r for n, r in report.items() if "%s%d," % (kernel, nv) in n}
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


@pytest.mark.parametrize("nv", FORMS)
def test_the_image_kernel_is_the_only_other_kernel_of_the_form(report, nv):
    """One more kernel per form builds the sweep's images; nothing of the file uses scratch."""
    assert sum("mlp_tiled_adj_image_kernel<%d>" % nv in n for n in report) == 1
    own = {n: r for n, r in report.items() if "tiled" in n and ("<%d," % nv in n or "<%d>" % nv in n)}
    assert len(own) == 32 + 16 + 1, sorted(own)
    assert all(r.get("ScratchSize [bytes/lane]") == "0" for r in own.values()), own
    assert sum("tiled" in n for n in report) == len(FORMS) * (32 + 16 + 1), sorted(report)
