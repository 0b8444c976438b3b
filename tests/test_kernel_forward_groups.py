"""K2bd's step loop as compiled (no GPU needed).  rk4_bf16x3_duo.hip is compiled to gfx950 assembly with the project's own
flags and the loop with 768 MFMAs -- one RK step: 4 stages x 2 groups x 16 tiles x 6 piece products -- is counted
(scripts/loop_counts.py); the compiler's resource report is read as in test_kernel_forward_resident_weights.py.

* every MFMA is a v_mfma_f32_16x16x32_bf16 and reads SrcA from the weight image in AGPRs (192 of them);
* the wave stays within its 256 VGPRs without scratch or spills;
* LDS reads: 4 stages x 2 groups x 16 bias tiles = 128 ds_read_b128, and the control exchange through the per-wave LDS
  strip adds two ds_read_b128 per group and stage (the lane's eight slopes; the write is one ds_write_b64): 144;
* the interleave: a phase is written as 96 slots of one MFMA and two vector instructions of the other group's contraction,
  update and split; that work is 132 to 164 instructions by stage, so a phase ends with 14 to 30 MFMAs with no vector
  instruction between them.  The kept build shows 30 as the longest such run; the bar is 30 + 2.  The same source built with
  -DBXD_INTERLEAVE=0 (each phase's vector work behind its MFMAs) shows 96."""
import importlib.util
import os
import re
import subprocess

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rk4_bf16x3_duo.hip"
KERNELS = ["rk4_forward_bf16x3_duo<float, 3>", "rk4_forward_bf16x3_duo<float, 1>", "rk4_forward_bf16x3_duo<double, 3>",
           "rk4_forward_bf16x3_duo<double, 1>"]
BARE_RUN_KEPT = 30


def _loop_counts():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    loop_counts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loop_counts)
    return loop_counts


@pytest.fixture(scope="module")
def step_loops():
    return _loop_counts().loop_table(os.path.join(_lib._CSRC, SRC), "rk4_forward_bf16x3_duo<", mfma=768)


@pytest.fixture(scope="module")
def resources():
    """kernel name (demangled, without arguments) -> the compiler's resource remarks for it"""
    flags = [f for f in _lib.HIPCC_FLAGS if f != "-shared"] + _lib.EXTRA_FLAGS.get(SRC, [])
    proc = subprocess.run([_lib._hipcc()] + flags + ["-c", os.path.join(_lib._CSRC, SRC), "-o", os.devnull,
                                                     "-Rpass-analysis=kernel-resource-usage"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout[-4000:]
    rows, cur = [], None
    for line in proc.stdout.splitlines():
        m = re.search(r"remark:\s+([^:]+): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = {"mangled": val}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    names = subprocess.run(["c++filt"] + [r["mangled"] for r in rows], stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {re.sub(r"\(.*", "", n).replace("void ", ""): r for r, n in zip(rows, names)}


def _one(table, kernel):
    found = [row for name, row in table.items() if name.endswith(kernel)]
    assert len(found) == 1, "kernels found: %s" % sorted(table)
    return found[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_step_loop_runs_on_16x16x32_with_weights_in_agprs(step_loops, kernel):
    row = _one(step_loops, kernel)
    print(kernel, row)
    assert row["mfma"] == 768 and row["mfma_16x16x32_bf16"] == 768, row
    assert row["mfma_srca_agpr"] == 768, row
    assert row["ds_read_b128"] <= 128 + 16, row
    assert row["scratch"] == 0, row


@pytest.mark.parametrize("kernel", KERNELS)
def test_step_loop_interleaves_the_groups(step_loops, kernel):
    row = _one(step_loops, kernel)
    print(kernel, row["mfma_run_max"])
    assert row["mfma_run_max"] <= BARE_RUN_KEPT + 2, row


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_holds_the_image_without_spilling(resources, kernel):
    r = _one(resources, kernel)
    print(kernel, r)
    assert int(r.get("AGPRs", "0")) >= 192 and int(r.get("VGPRs", "999")) <= 256, r
    assert r.get("ScratchSize [bytes/lane]") == "0" and r.get("VGPRs Spill") == "0", r
