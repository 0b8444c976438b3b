"""The default path's kernels stay out of scratch (no GPU needed): the headline solve's kernels are compiled for gfx950 with
the project's own flags and the compiler's resource report is read.  A spill on the chain wave of K3p costs scratch traffic
on the critical path of every stage, and it comes back quietly with a compiler flag or a few more live registers."""
import os
import re
import subprocess

import pytest

from torchcde_amd import _lib


def _resources(src):
    """kernel name (demangled, without arguments) -> the compiler's resource remarks for it"""
    path = os.path.join(_lib._CSRC, src)
    flags = [f for f in _lib.HIPCC_FLAGS if f != "-shared"] + _lib.EXTRA_FLAGS.get(src, [])
    proc = subprocess.run([_lib._hipcc()] + flags + ["-c", path, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
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
    out = {}
    for r, n in zip(rows, names):
        n = re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "")).replace("void ", "")
        out[n] = r
    return out


@pytest.mark.parametrize("src,kernel", [
    ("rk4_adjoint_pair.hip", "rk4_adjoint_jacobian_pair<"),   # K3p, every instantiation (bf16 and f32 forms, f32 / f64 time)
    ("rk4_bf16x3.hip", "rk4_forward_bf16x3<"),                # K2b
])
def test_default_path_kernels_use_no_scratch(src, kernel):
    found = {n: r for n, r in _resources(src).items() if kernel in n}
    assert found, "no %s kernels in %s" % (kernel, src)
    spilled = {n: (r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill")) for n, r in found.items()
               if r.get("ScratchSize [bytes/lane]") != "0" or r.get("VGPRs Spill") != "0"}
    assert not spilled, "scratch (bytes per lane, spilled VGPRs): %s" % spilled
    if "pair" in kernel:                      # two waves per SIMD (chain + helper) need <= 256 registers
        assert all(int(r["VGPRs"]) + int(r.get("AGPRs", "0")) <= 256 for r in found.values())
