"""K2b keeps its weight pieces in accumulator registers (no GPU needed).  rk4_bf16x3.hip is compiled to gfx950 assembly with
the project's own flags and the loop with the most MFMAs -- one RK step, four stages -- is counted (scripts/loop_counts.py);
the compiler's resource report is read as in test_kernel_resources.py.

The piece image of the weights is loop invariant: 8 tiles x 2 K steps x 3 pieces, one uint4 per lane each, 192 registers.
K2b runs one wave per SIMD and owns all 512 registers of it, so the image sits in AGPRs for the whole solve and every MFMA
reads SrcA from there.  What the step still reads from LDS is the bias table: 4 stages x 8 tiles x 4 ds_read_b128 = 128.  Read
from LDS in every stage, as before, the step held 320 ds_read_b128 and 24 AGPRs (spill slots)."""
import importlib.util
import os
import re
import subprocess

import pytest

from torchcde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "rk4_bf16x3.hip"
KERNELS = ["rk4_forward_bf16x3<float, 3>", "rk4_forward_bf16x3<float, 1>", "rk4_forward_bf16x3<double, 3>",
           "rk4_forward_bf16x3<double, 1>"]


@pytest.fixture(scope="module")
def step_loops():
    spec = importlib.util.spec_from_file_location("loop_counts", os.path.join(ROOT, "scripts", "loop_counts.py"))
    loop_counts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(loop_counts)
    return loop_counts.loop_table(os.path.join(_lib._CSRC, SRC), "rk4_forward_bf16x3<")


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
def test_forward_step_reads_its_weights_from_agprs(step_loops, kernel):
    row = _one(step_loops, kernel)
    print(kernel, row)
    assert row["mfma"] == 384 and row["mfma_32x32x16_bf16"] == 384, row       # 4 stages x 8 tiles x 2 K steps x 6 pieces
    assert row["mfma_srca_agpr"] == 384, row
    assert row["ds_read_b128"] <= 160, row                                    # 128 bias reads + slack for the control path


@pytest.mark.parametrize("kernel", KERNELS)
def test_forward_kernel_holds_the_image_without_spilling(resources, kernel):
    r = _one(resources, kernel)
    print(kernel, r)
    assert int(r.get("AGPRs", "0")) >= 192, r
    assert r.get("ScratchSize [bytes/lane]") == "0" and r.get("VGPRs Spill") == "0", r
