"""Instruction classes of a kernel's hottest loop (no GPU needed): the translation unit is compiled to gfx950 assembly with
the project's own flags, and in each kernel whose name contains the filter the innermost loop that holds the most MFMAs is
counted -- for the fixed-grid solvers that is one RK step.
    python scripts/loop_counts.py torchcde_amd/csrc/rk4_bf16x3.hip 'rk4_forward_bf16x3<' [--mfma N] [flags in place of the file's own]
A loop is the span from a label to the last branch back to it, so the count is static: both sides of a branch inside the
loop are counted once each.  `--mfma N` takes the loop with exactly N MFMAs instead of the one with the most (the helper
wave's stage loop of rk4_adjoint_pair.hip has 96).  Beside the instruction classes the table counts the MFMAs whose SrcA is
read from AGPRs (`a[...]` as second operand, whatever the MFMA's shape), the longest run of MFMAs with no other vector
instruction between them (`mfma_run_max`), the LDS reads and waits of the loop, and `lds_cover_min` / `lds_wait_cover_min`: how far
ahead of the waits for them the LDS operands are requested (see lds_cover; `-` = the loop has no such wait), and
`vm_wait_cover_min` / `global_load_site_max`: the same for the loop's global loads (see vm_wait_cover)."""
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
        name = name.replace("(anonymous namespace)::", "")      # its parenthesis is not the argument list's
        out[re.sub(r"\(.*", "", name).replace("void ", "")] = lines
    return out


def hottest_loop(lines, mfma=None):
    """the instructions of the shortest label-to-back-branch span among those with the most MFMAs, or with exactly `mfma`"""
    at = {ln: i for i, ln in enumerate(lines) if ln.startswith(".LBB")}
    last_back = {}
    for i, ln in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            last_back[m.group(1)] = i
    best = None
    for label, end in last_back.items():
        body = [ln for ln in lines[at[label]:end + 1] if not ln.startswith(".LBB")]
        count = sum(ln.startswith("v_mfma") for ln in body)
        if mfma is not None and count != mfma:
            continue
        key = (-count, len(body))
        if best is None or key < best[0]:
            best = (key, body)
    return best[1] if best else []


def lds_cover(body, gating_only=True, mfma_only=False):
    """For every s_waitcnt with an lgkmcnt field whose next instruction other than s_nop is an MFMA (a wait that gates the
    matrix pipe): the number of MFMA and VALU instructions between the wait and the nearest ds_read* before it -- the work
    that covers the LDS round trip.  Waits with no ds_read before them in the loop body are left out.  gating_only=False
    takes every wait with an lgkmcnt field, whatever follows it (a wait that gates the wave); mfma_only=True counts the
    MFMAs alone."""
    cover = []
    for i, ln in enumerate(body):
        if not (ln.startswith("s_waitcnt") and "lgkmcnt" in ln):
            continue
        nxt = next((b for b in body[i + 1:] if not b.startswith("s_nop")), "")
        if gating_only and not nxt.startswith("v_mfma"):
            continue
        n = 0
        for b in reversed(body[:i]):
            if b.startswith("ds_read"):
                cover.append(n)
                break
            n += b.startswith("v_mfma") if mfma_only else b.startswith("v_")
    return cover


def vm_wait_cover(body):
    """For every s_waitcnt with a vmcnt field, the loop body taken as circular: the number of MFMAs between the wait and the
    nearest global_load_* before it -- the matrix work a memory request has had to arrive under before the wave may stop
    for it (vmcnt is one in-order counter: behind a branch the compiler waits for every load in flight, so a wait next to
    a request drains it on the spot).  Empty when the loop has no such wait or no global load."""
    if not any(b.startswith("global_load") for b in body):
        return []
    cover = []
    for i, ln in enumerate(body):
        if not (ln.startswith("s_waitcnt") and "vmcnt" in ln):
            continue
        n = 0
        for b in reversed(body[i + 1:] + body[:i]):
            if b.startswith("global_load"):
                cover.append(n)
                break
            n += b.startswith("v_mfma")
    return cover


def global_load_site_max(body):
    """the most global_load_* between two successive MFMAs of the loop (circular): the loads of one request site"""
    first = next((i for i, b in enumerate(body) if b.startswith("v_mfma")), 0)
    run = best = 0
    for b in body[first:] + body[:first]:
        if b.startswith("v_mfma"):
            run = 0
        elif b.startswith("global_load"):
            run += 1
            best = max(best, run)
    return best


def mfma_run_max(op):
    """the longest run of MFMAs with no other vector instruction between them (waits, s_nop and LDS reads do not end a run)"""
    run = best = 0
    for o in op:
        if o.startswith("v_mfma"):
            run += 1
            best = max(best, run)
        elif o.startswith("v_"):
            run = 0
    return best


def classes(body):
    op = [re.sub(r"_(e32|e64|dpp|sdwa)$", "", ln.split()[0]) for ln in body]
    valu = [o for o in op if o.startswith("v_") and not o.startswith("v_mfma")]
    return {"instructions": len(op), "mfma": sum(o.startswith("v_mfma") for o in op),
            "mfma_32x32x16_bf16": sum(o == "v_mfma_f32_32x32x16_bf16" for o in op),
            "mfma_16x16x32_bf16": sum(o == "v_mfma_f32_16x16x32_bf16" for o in op), "mfma_run_max": mfma_run_max(op),
            "valu": len(valu),
            "v_accvgpr_read_b32": op.count("v_accvgpr_read_b32"), "v_accvgpr_write_b32": op.count("v_accvgpr_write_b32"),
            "v_mov_b32": op.count("v_mov_b32"), "copies": sum(op.count(c) for c in COPIES),
            "v_pk_fma_f32": op.count("v_pk_fma_f32"), "v_pk_mul_f32": op.count("v_pk_mul_f32"),
            "v_pk_add_f32": op.count("v_pk_add_f32"), "v_pk": sum(o.startswith("v_pk_") for o in op),
            "v_readlane_b32": op.count("v_readlane_b32"),
            "branches": sum(o.startswith("s_cbranch") or o == "s_branch" for o in op),
            "scratch": sum(o.startswith("scratch_") for o in op),
            "ds_read_b128": op.count("ds_read_b128"), "lds_reads": sum(o.startswith("ds_read") for o in op),
            "s_waitcnt": op.count("s_waitcnt"), "lds_cover_min": min(lds_cover(body), default=None),
            "lds_wait_cover_min": min(lds_cover(body, gating_only=False), default=None),
            "global_load": sum(o.startswith("global_load") for o in op), "global_load_site_max": global_load_site_max(body),
            "vm_wait_cover_min": min(vm_wait_cover(body), default=None),
            # MFMAs whose SrcA (the second operand) is read straight from accumulator registers
            "mfma_srca_agpr": sum(bool(re.match(r"v_mfma\S*\s+[^,]+,\s*a\[", ln)) for ln in body)}


def loop_bodies(src, name_filter="", extra_flags=None, mfma=None):
    return {n: hottest_loop(lines, mfma) for n, lines in kernels(assembly(src, extra_flags)).items() if name_filter in n}


def loop_table(src, name_filter="", extra_flags=None, mfma=None):
    return {n: classes(body) for n, body in loop_bodies(src, name_filter, extra_flags, mfma).items()}


if __name__ == "__main__":
    rest, mfma = sys.argv[3:], None
    if rest[:1] == ["--mfma"]:
        mfma, rest = int(rest[1]), rest[2:]
    table = loop_table(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "", rest or None, mfma)
    cols = ["instructions", "mfma", "mfma_16x16x32_bf16", "mfma_srca_agpr", "mfma_run_max", "valu", "copies", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_mov_b32",
            "v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32", "v_pk", "v_readlane_b32", "ds_read_b128", "s_waitcnt", "lds_cover_min", "lds_wait_cover_min", "global_load", "global_load_site_max", "vm_wait_cover_min",
            "branches", "scratch"]
    print(" ".join("%-12s" % c[-12:] for c in cols) + " kernel")
    for n, row in table.items():
        print(" ".join("%-12s" % ("-" if row[c] is None else row[c]) for c in cols) + " " + n.replace("cde::", ""))
