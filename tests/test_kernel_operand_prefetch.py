"""K3p's helper wave requests its LDS operands a block ahead of the splits that wait for them (no GPU needed).
rk4_adjoint_pair.hip is compiled to gfx950 assembly with the project's own flags and the helper's stage loop of the bf16
form -- the loop with 96 MFMAs: 2 K blocks x 8 channels x 6 piece products -- is read with scripts/loop_counts.py.

Each of the 16 blocks of a stage multiplies the weighted control derivative of its channel into a^T, splits the products
into bf16 pieces and issues six MFMAs.  Requested where it is used, the derivative (two ds_read_b128) was waited for at
once, 16 LDS round trips per stage in front of the splits.  Requested before the previous block's MFMAs -- at the last
channel of a K block together with the next K block's z / a rows, and the stage's first block before the wave forms the
control derivative of a later stage -- every wait that holds the wave back finds its reads at least six MFMAs old.  The
loop's first waits have no read before them in the loop (the stage's first requests are issued in front of it).

K2b's bias tiles a pair ahead (`lds_cover_min` >= 24 in its step loop) and the chain wave's first row images in front of
the stage barrier were built and measured too, and not kept: neither moved its kernel's time (profiles/NOTES.md, round 11),
so this file holds no bar for them."""
import importlib.util
import os

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPER_KERNELS = ["rk4_adjoint_jacobian_pair<float, 3, 0, true>", "rk4_adjoint_jacobian_pair<float, 1, 0, true>"]


@pytest.fixture(scope="module")
def loop_counts():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def helper_loops(loop_counts):
    return loop_counts.loop_bodies(os.path.join(_lib._CSRC, "rk4_adjoint_pair.hip"), "rk4_adjoint_jacobian_pair<", mfma=96)


@pytest.mark.parametrize("kernel", HELPER_KERNELS)
def test_helper_requests_its_operands_a_block_ahead(loop_counts, helper_loops, kernel):
    found = [body for name, body in helper_loops.items() if name.endswith(kernel)]
    assert len(found) == 1, "kernels found: %s" % sorted(helper_loops)
    body = found[0]
    row = loop_counts.classes(body)
    print(kernel, row)
    assert row["mfma"] == 96 and row["mfma_32x32x16_bf16"] == 96, row         # the helper's stage, not another loop
    assert row["ds_read_b128"] == 34 and row["scratch"] == 0, row             # 16 x 2 derivative reads + the second K block's z, a rows
    cover = loop_counts.lds_cover(body, gating_only=False, mfma_only=True)
    print(kernel, cover)
    assert len(cover) >= 30 and min(cover) >= 6, cover                        # two waits per block from the second block on


def test_lds_cover_counts_from_the_nearest_read(loop_counts):
    body = ["ds_read_b128 v[0:3], v9", "v_add_f32_e32 v8, v8, v8", "s_waitcnt lgkmcnt(0)", "s_nop 1",
            "v_mfma_f32_32x32x16_bf16 v[0:15], a[0:3], v[20:23], v[0:15]", "ds_read_b128 v[4:7], v9",
            "v_mfma_f32_32x32x16_bf16 v[0:15], a[0:3], v[20:23], v[0:15]", "v_mov_b32_e32 v8, 0", "s_mov_b32 s0, 0",
            "s_waitcnt vmcnt(0)", "s_waitcnt vmcnt(0) lgkmcnt(0)", "v_mov_b32_e32 v8, v4", "s_waitcnt lgkmcnt(0)",
            "ds_read_b128 v[4:7], v9"]
    assert loop_counts.lds_cover(body) == [1]                                 # the first wait gates an MFMA, one VALU after its read
    assert loop_counts.lds_cover(body, gating_only=False) == [1, 2, 3]        # every lgkmcnt wait; vmcnt alone is none
    assert loop_counts.lds_cover(body, gating_only=False, mfma_only=True) == [0, 1, 1]
    assert loop_counts.lds_cover(body[2:5]) == []                             # no read before the wait in the body
    row = loop_counts.classes(body)
    assert row["lds_cover_min"] == 1 and row["lds_wait_cover_min"] == 1
    assert loop_counts.classes(body[5:8])["lds_cover_min"] is None


def test_a_loop_is_selected_by_its_mfma_count(loop_counts):
    lines = [".LBB0_1", "v_mfma_f32_32x32x16_bf16 v[0:15], a[0:3], v[20:23], v[0:15]", "s_cbranch_scc1 .LBB0_1",
             ".LBB0_2", "v_mfma_f32_32x32x16_bf16 v[0:15], a[0:3], v[20:23], v[0:15]",
             "v_mfma_f32_32x32x16_bf16 v[0:15], a[0:3], v[20:23], v[0:15]", "s_cbranch_scc1 .LBB0_2"]
    assert len(loop_counts.hottest_loop(lines)) == 3                          # the default: most MFMAs
    assert len(loop_counts.hottest_loop(lines, mfma=1)) == 2
    assert loop_counts.hottest_loop(lines, mfma=5) == []
