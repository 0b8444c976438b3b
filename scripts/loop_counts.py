"""Instruction classes of a kernel's hottest loop (no GPU needed): the translation unit is compiled to gfx950 assembly with
the project's own flags, and in each kernel whose name contains the filter the innermost loop that holds the most MFMAs is
counted -- for the fixed-grid solvers that is one RK step.
    python scripts/loop_counts.py torchcde_amd/csrc/rk4_bf16x3.hip 'rk4_forward_bf16x3<' [flags in place of the file's own]
A loop is the span from a label to the last branch back to it, so the count is static: both sides of a branch inside the
loop are counted once each.  Beside the instruction classes the table counts the MFMAs whose SrcA is read from AGPRs
(`a[...]` as second operand) and the LDS reads and waits of the loop."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torchcde_amd import _lib  # noqa: E402

COPIES = ("v_mov_b32", "v_accvgpr_read_b32", "v_accvgpr_write_b32")      # the assembler prints v_mov_b32_e32 and its kin


def assembly(src, extra_flags=None):
    """gfx950 assembly of one source of torchcde_amd/csrc, built with _lib.HIPCC_FLAGS + _lib.EXTRA_FLAGS for it"""
    src = os.path.abspath(src)
    extra = _lib.EXTRA_FLAGS.get(os.path.basename(src), []) if extra_flags is None else extra_flags
    flags = [f for f in _lib.HIPCC_FLAGS if f != "-shared"] + extra
    proc = subprocess.run([_lib._hipcc()] + flags + ["--cuda-device-only", "-S", src, "-o", "-"], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True)
    if proc.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + proc.stderr[-4000:])
    return proc.stdout


def kernels(text):
    """demangled kernel name (without arguments) -> its instruction lines and labels, in order"""
    parts = re.split(r"\n(_Z\w+):", text)
    names = subprocess.run(["c++filt"] + parts[1::2], stdout=subprocess.PIPE, text=True).stdout.splitlines()
    out = {}
    for name, body in zip(names, parts[2::2]):
        body = body.split(".Lfunc_end")[0]
        lines = []
        for ln in body.split("\n"):
            m = re.match(r"(\.LBB\d+_\d+):", ln)
            if m:
                lines.append(m.group(1))
            elif ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;"):
                lines.append(ln.strip())
        out[re.sub(r"\(.*", "", name).replace("void ", "")] = lines
    return out


def hottest_loop(lines):
    """the instructions of the shortest label-to-back-branch span among those with the most MFMAs"""
    at = {ln: i for i, ln in enumerate(lines) if ln.startswith(".LBB")}
    last_back = {}
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            last_back[m.group(1)] = i
    best = None
    for label, end in last_back.items():
        body = [ln for ln in lines[at[label]:end + 1] if not ln.startswith(".LBB")]
        key = (-sum(ln.startswith("v_mfma") for ln in body), len(body))
        if best is None or key < best[0]:
            best = (key, body)
    return best[1] if best else []


def classes(body):
    op = [re.sub(r"_(e32|e64|dpp|sdwa)$", "", ln.split()[0]) for ln in body]
    valu = [o for o in op if o.startswith("v_") and not o.startswith("v_mfma")]
    return {"instructions": len(op), "mfma": sum(o.startswith("v_mfma") for o in op),
            "mfma_32x32x16_bf16": sum(o == "v_mfma_f32_32x32x16_bf16" for o in op), "valu": len(valu),
            "v_accvgpr_read_b32": op.count("v_accvgpr_read_b32"), "v_accvgpr_write_b32": op.count("v_accvgpr_write_b32"),
            "v_mov_b32": op.count("v_mov_b32"), "copies": sum(op.count(c) for c in COPIES),
            "v_pk_fma_f32": op.count("v_pk_fma_f32"), "v_readlane_b32": op.count("v_readlane_b32"),
            "branches": sum(o.startswith("s_cbranch") or o == "s_branch" for o in op),
            "scratch": sum(o.startswith("scratch_") for o in op),
            "ds_read_b128": op.count("ds_read_b128"), "lds_reads": sum(o.startswith("ds_read") for o in op),
            "s_waitcnt": op.count("s_waitcnt"),
            # MFMAs whose SrcA (the second operand) is read straight from accumulator registers
            "mfma_srca_agpr": sum(bool(re.match(r"v_mfma\S*\s+[^,]+,\s*a\[", ln)) for ln in body)}


def loop_table(src, name_filter="", extra_flags=None):
    return {n: classes(hottest_loop(lines)) for n, lines in kernels(assembly(src, extra_flags)).items() if name_filter in n}


if __name__ == "__main__":
    table = loop_table(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "", sys.argv[3:] or None)
    cols = ["instructions", "mfma", "mfma_srca_agpr", "valu", "copies", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_mov_b32",
            "v_pk_fma_f32", "v_readlane_b32", "ds_read_b128", "s_waitcnt", "branches", "scratch"]
    print(" ".join("%-12s" % c[-12:] for c in cols) + " kernel")
    for n, row in table.items():
        print(" ".join("%-12d" % row[c] for c in cols) + " " + n.replace("cde::", ""))
