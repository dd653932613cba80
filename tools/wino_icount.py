#!/usr/bin/env python3
"""Static instruction counts of the Winograd kernels by region (no GPU needed).

Compiles csrc/i2r_conv_wino.hip device-only to gfx950 assembly, takes every kernel of it, splits its text at the workgroup barriers and
prints, per region, how many instructions of each class it holds.  The classes go by mnemonic prefix only: MFMA, other vector ALU, LDS,
vector memory, scalar loads, waits / nops, branches, other scalar.

The counts are STATIC: a region holds every block the compiler laid out there, taken or not (the general epilogue, form 0, carries
its untaken res2 / res_post / tail blocks; the forms 1 and 2 have no branch in their epilogue, so there the static count is the executed
one).  The text is split at the barriers and at the loop over the fragments of a run (its first block in the text and its header), so
the run's set-up stands alone.  The compiler lays the loop out differently per form; the regions of a kernel, in text order:
    form 0:       run set-up | closing blocks of the epilogue | fragment set-up | staging store of chunk 0 | first pass | further pass |
                  output transform over j + index math + bias / residual loads (to the exchange barrier) | over i + epilogue
    forms 1, 2:   run set-up | output transform over j + index math + loads (to the exchange barrier) | over i + epilogue |
                  fragment set-up | staging store of chunk 0 | first pass | further pass | end of the kernel
The plain form's pass exists in four copies since its load schedule became explicit (first | middle, whose closing barrier the rotated
loop puts ABOVE its body in the text | last | only), so there the pass regions are more and the middle one is split in two;
tools/wino_sched.py names the pass regions by what they hold and reads their load / wait schedule.
usage: tools/wino_icount.py [--match conv_wino_f32<1, 3] [--src other/i2r_conv_wino.hip] [--json out.json] [extra hipcc flags]
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc")
CLASSES = ("mfma", "valu", "lds", "vmem", "smem", "wait", "branch", "salu")


def classify(m):
    if m.startswith("v_mfma") or m.startswith("v_smfma"):
        return "mfma"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "smem"
    if m.startswith(("s_waitcnt", "s_nop", "s_sleep")):
        return "wait"
    if m.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")):
        return "branch"
    if m.startswith("v_"):
        return "valu"
    return "salu"


def kernels(asm):
    """-> {demangled kernel name: [mnemonic, ...]} of the .amdhsa_kernel functions of an assembly text"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    out = {}
    for sym in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.Lfunc_end\d+:" % re.escape(sym), asm, flags=re.M | re.S)
        if not m:
            continue
        ins = []
        for line in m.group(1).splitlines():
            if re.match(r"\.LBB\d+_\d+:.*This Loop Header: Depth=1", line) or ("@loop" not in ins and re.match(r"\.LBB\d+_\d+:.*in Loop: Header=\S+ Depth=1", line)):
                ins.append("@loop")  # (the loop over the fragments of a run: its first block in the text, and its header)
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            ins.append(line.split()[0])
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", dem)] = ins
    return out


def regions(ins):
    """split at s_barrier and at the head of the run loop -> list of {class: count}; the barrier itself is counted with the region it closes (other scalar)"""
    regs, cur = [], dict.fromkeys(CLASSES, 0)
    for m in ins:
        if m != "@loop":
            cur[classify(m)] += 1
        if m.startswith("s_barrier") or m == "@loop":
            regs.append(cur)
            cur = dict.fromkeys(CLASSES, 0)
    regs.append(cur)
    return regs


def main(argv):
    src, match, out_json, extra = os.path.join(CSRC, "i2r_conv_wino.hip"), "conv_wino", None, []
    it = iter(argv)
    for a in it:
        if a == "--src":
            src = next(it)
        elif a == "--match":
            match = next(it)
        elif a == "--json":
            out_json = next(it)
        else:
            extra.append(a)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "wino.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form",
                               "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-I", CSRC, "--cuda-device-only", "-S", src, "-o", s] + extra)
        asm = open(s).read()
    result = {}
    for name, ins in sorted(kernels(asm).items()):
        if match not in name:
            continue
        regs = regions(ins)
        result[name] = regs
        print("%s: %d instructions, %d regions" % (name, len(ins), len(regs)))
        print("  region " + " ".join("%6s" % c for c in CLASSES) + "   non-MFMA")
        for i, r in enumerate(regs):
            print("  %6d " % i + " ".join("%6d" % r[c] for c in CLASSES) + "   %8d" % (sum(r.values()) - r["mfma"]))
    if out_json:
        json.dump(result, open(out_json, "w"), indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
