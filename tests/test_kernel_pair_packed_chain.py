"""K3p's bf16 form takes the chain wave's J-row consume as packed f32 (no GPU needed).  rk4_adjoint_pair.hip is compiled to
gfx950 assembly with the project's own flags, as test_kernel_operand_prefetch.py does, and the chain wave's step loop -- the
loop with 396 MFMAs: 4 stages x 33 rows x 3 piece products -- is read with scripts/loop_counts.py.

A stage consumes 32 rows of J; each consume is 16 FMAs into the row's four partial sums of f_h and 16 into a^T J.  On the
adjacent register pairs (J[2j], J[2j + 1]), (z[2j], z[2j + 1]), (vs[2j], vs[2j + 1]) that is 16 v_pk_fma_f32 per row, a_h
broadcast by op_sel: 4 x 32 x 16 = 2,048 per step in place of 4,096 v_fma_f32.  The two SIMD-sharing waves of this kernel are
bound by instruction issue, not by the matrix pipe (profiles/NOTES.md, round 12), so the issue slots are what counts.

Bars, the chain's step loop: 396 MFMAs; exactly 2,048 v_pk_fma_f32; 128 v_pk_add_f32 (one per consumed row: p + q) and no
v_pk_mul_f32 -- the sum of a row's two halves stays a scalar add (left to the compiler it becomes a second v_pk_add_f32 per
row, 280 in all, which measured 0.02 ms slower), and the 3/8-rule update stays scalar; at most 4,836 + 8 instructions, 4,836
being what the kept build shows for both control degrees (scripts/loop_counts.py on the committed file with the project's
flags; 8 of slack for a scheduler's moves and waits; the scalar form of the build before round 12 shows 6,886, and each
packed FMA takes the place of two scalar ones); no scratch.  The build before round 12 fails with 0 packed FMAs and 6,886
instructions.

Built, measured and not kept (profiles/NOTES.md, round 12): the 3/8-rule update as packed arithmetic -- written pair by pair
it spills, written on whole f32x16 values it gains 0.014 ms on the kernel and nothing the step's timing resolves -- and the
helper wave's products and split remainders as v_pk_mul_f32 / v_pk_add_f32 (slower than no packing at all).  The helper's
stage loop therefore stays free of packed f32, which test_helper_stays_on_scalar_f32 pins."""
import importlib.util
import os

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["rk4_adjoint_jacobian_pair<float, 3, 0, true>", "rk4_adjoint_jacobian_pair<float, 1, 0, true>"]


@pytest.fixture(scope="module")
def loop_counts():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def kernel_lines(loop_counts):
    text = loop_counts.assembly(os.path.join(_lib._CSRC, "rk4_adjoint_pair.hip"))
    return {n: lines for n, lines in loop_counts.kernels(text).items() if "rk4_adjoint_jacobian_pair<" in n}


def _loop(loop_counts, kernel_lines, kernel, mfma):
    found = [lines for name, lines in kernel_lines.items() if name.endswith(kernel)]
    assert len(found) == 1, "kernels found: %s" % sorted(kernel_lines)
    return loop_counts.classes(loop_counts.hottest_loop(found[0], mfma))


@pytest.mark.parametrize("kernel", KERNELS)
def test_chain_consumes_its_rows_with_packed_fmas(loop_counts, kernel_lines, kernel):
    row = _loop(loop_counts, kernel_lines, kernel, 396)
    print(kernel, row)
    assert row["mfma"] == 396 and row["mfma_32x32x16_bf16"] == 396, row       # the chain's RK step, not another loop
    assert row["v_pk_fma_f32"] == 2048, row
    assert row["v_pk_add_f32"] == 128 and row["v_pk_mul_f32"] == 0 and row["v_pk"] == 2048 + 128, row
    assert row["instructions"] <= 4836 + 8, row
    assert row["scratch"] == 0, row


@pytest.mark.parametrize("kernel", KERNELS)
def test_helper_stays_on_scalar_f32(loop_counts, kernel_lines, kernel):
    row = _loop(loop_counts, kernel_lines, kernel, 96)
    print(kernel, row)
    assert row["mfma"] == 96 and row["ds_read_b128"] == 34, row
    assert row["v_pk"] == 0, row


def test_classes_counts_packed_f32():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    body = ["v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[0:1] op_sel_hi:[1,0,1]", "v_pk_mul_f32 v[0:1], v[2:3], v[4:5]",
            "v_pk_add_f32 v[0:1], v[2:3], v[4:5] neg_lo:[0,1] neg_hi:[0,1]", "v_pk_add_f32 v[0:1], v[2:3], v[4:5]",
            "v_fma_f32 v0, v1, v2, v0", "v_cvt_pk_bf16_f32 v0, v1, v2"]
    row = module.classes(body)
    assert (row["v_pk_fma_f32"], row["v_pk_mul_f32"], row["v_pk_add_f32"], row["v_pk"]) == (1, 1, 2, 4), row
    assert row["valu"] == 6
