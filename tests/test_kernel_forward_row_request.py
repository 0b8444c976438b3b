"""K2bd's control-row request as compiled (no GPU needed).  rk4_bf16x3_duo.hip is compiled to gfx950 assembly with the project's
own flags and the 768-MFMA step loop is read with scripts/loop_counts.py, as tests/test_kernel_forward_groups.py does.

The wave has one in-order counter for its global loads (vmcnt), and the row request sits behind a uniform branch (it is made
only where the interval index changes), so the compiler cannot know how many loads are in flight behind it: the first read
of ANY row register after the branch becomes `s_waitcnt vmcnt(0)`, a wait for every request issued so far.  With the request at
the tail of a phase that wait -- the next phase's slope write, on the other group's row -- stood about ten instructions
behind the request and drained it on the spot: a full memory round trip on the SIMD's only wave with the matrix pipe idle,
where the index changes (once per RK step and group on unit-spaced knots under step 1).

* `vm_wait_cover_min`: for every wait with a vmcnt field in the step loop (body taken as circular), the MFMAs between the wait
  and the nearest global load before it; the minimum over the waits.  The request now stands at the head of the phase, behind
  the slope write that last reads its registers, so every such wait has the phase's 96 MFMAs (>= 1,536 cycles) behind the
  newest request; the bar is 80.  The request at the tail (-DBXD_ROW_AT_TAIL=1, kept for A/B timing) gives 0.
* the request itself is unchanged: six dword loads per site and lane (four for a linear control), one site per phase.  The
  branch-free form of three 8-byte loads was built and timed, gained nothing beyond the placement and was taken out
  (profiles/NOTES.md, round 14), and with it its bar of three loads per site.
* nothing else moved: the pins of test_kernel_forward_groups.py are asserted there, on the same build."""
import importlib.util
import os

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rk4_bf16x3_duo.hip"
KERNELS = ["rk4_forward_bf16x3_duo<float, 3>", "rk4_forward_bf16x3_duo<float, 1>", "rk4_forward_bf16x3_duo<double, 3>",
           "rk4_forward_bf16x3_duo<double, 1>"]
COVER_BAR = 80


def _loop_counts():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    loop_counts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loop_counts)
    return loop_counts


@pytest.fixture(scope="module")
def step_loops():
    return _loop_counts().loop_table(os.path.join(_lib._CSRC, SRC), "rk4_forward_bf16x3_duo<", mfma=768)


@pytest.fixture(scope="module")
def step_loops_row_at_tail():
    flags = _lib.EXTRA_FLAGS[SRC] + ["-DBXD_ROW_AT_TAIL=1"]
    return _loop_counts().loop_table(os.path.join(_lib._CSRC, SRC), "rk4_forward_bf16x3_duo<float, 3>", flags, mfma=768)


def _one(table, kernel):
    found = [row for name, row in table.items() if name.endswith(kernel)]
    assert len(found) == 1, "kernels found: %s" % sorted(table)
    return found[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_wait_for_memory_has_a_phase_of_mfmas_behind_the_newest_request(step_loops, kernel):
    row = _one(step_loops, kernel)
    print(kernel, "vm_wait_cover_min", row["vm_wait_cover_min"], "global_load", row["global_load"])
    assert row["mfma"] == 768 and row["global_load"] > 0, row
    assert row["vm_wait_cover_min"] is not None and row["vm_wait_cover_min"] >= COVER_BAR, row


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_request_site_per_phase(step_loops, kernel):
    row = _one(step_loops, kernel)
    print(kernel, "global_load_site_max", row["global_load_site_max"], "global_load", row["global_load"])
    assert 1 <= row["global_load_site_max"] <= 6 and row["global_load"] <= 8 * 6, row
    assert row["scratch"] == 0, row


def test_the_switch_rebuilds_the_request_at_the_tail(step_loops_row_at_tail):
    """the measure sees the form it was written against: the A/B build drains its request where it is issued"""
    row = _one(step_loops_row_at_tail, KERNELS[0])
    print("BXD_ROW_AT_TAIL=1", row["vm_wait_cover_min"], row["global_load_site_max"])
    assert row["mfma"] == 768 and row["scratch"] == 0, row
    assert row["vm_wait_cover_min"] == 0 and row["global_load_site_max"] == 6, row


def test_the_measure_on_a_written_loop():
    """vm_wait_cover / global_load_site_max on a loop body written out: circular, nearest load, MFMAs only"""
    lc = _loop_counts()
    mfma, valu = "v_mfma_f32_16x16x32_bf16 v[0:3], a[0:3], v[4:7], v[0:3]", "v_add_f32_e32 v1, v2, v3"
    load, wait = "global_load_dwordx2 v[8:9], v[10:11], off", "s_waitcnt vmcnt(0)"
    body = [wait, valu, load, load] + [mfma, valu] * 5 + [wait] + [mfma] * 2        # second wait: 5 behind; first: 7, circular
    assert sorted(lc.vm_wait_cover(body)) == [5, 7]
    assert lc.global_load_site_max(body) == 2
    assert lc.vm_wait_cover([mfma, "s_waitcnt lgkmcnt(0)", load, mfma]) == []       # no wait with a vmcnt field
    assert lc.vm_wait_cover([mfma, wait, mfma]) == []                              # no load to wait for
    assert lc.vm_wait_cover([load, "s_waitcnt vmcnt(0) lgkmcnt(0)", mfma]) == [0]
