"""K2b's RK step is not dominated by register copies (no GPU needed).  rk4_bf16x3.hip is compiled to gfx950 assembly with
the project's own flags and the loop with the most MFMAs -- one RK step, four stages -- is counted (scripts/loop_counts.py).

K2b runs one wave per SIMD, and a wave hides next to nothing behind its own MFMAs, so every instruction of the step is
kernel time.  Built without -amdgpu-mfma-vgpr-form, and with the two units of a Y tile eight accumulator registers apart,
the step held 1,019 and more v_mov / v_accvgpr_read / v_accvgpr_write against its 384 MFMAs; with both it holds 191-270.
The bar -- fewer copies than MFMAs -- says that copies are no longer the step's largest class, and leaves the compiler
room."""
import importlib.util
import os

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def step_loops():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    loop_counts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loop_counts)
    return loop_counts.loop_table(os.path.join(_lib._CSRC, "rk4_bf16x3.hip"), "rk4_forward_bf16x3<")


@pytest.mark.parametrize("kernel", ["rk4_forward_bf16x3<float, 3>", "rk4_forward_bf16x3<float, 1>"])
def test_forward_step_has_fewer_register_copies_than_mfmas(step_loops, kernel):
    found = [row for name, row in step_loops.items() if name.endswith(kernel)]
    assert len(found) == 1, "kernels found: %s" % sorted(step_loops)
    row = found[0]
    print(kernel, row)
    assert row["mfma"] == 384 and row["mfma_32x32x16_bf16"] == 384, row       # 4 stages x 8 tiles x 2 K steps x 6 pieces
    assert row["copies"] < row["mfma"], row
