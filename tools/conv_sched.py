#!/usr/bin/env python3
"""Static load / wait schedule of the direct fp32 conv's K loop (conv_igemm_f32 in csrc/i2r_conv.hip; no GPU needed).

On the model of tools/wino_sched.py (same compile line, same in-order vmcnt model), but the chunk of this kernel is not one straight
region: a two-steps-per-trip loop and three tails (3, 2 or 1 steps left), chosen at run time.  So the unit here is the BASIC BLOCK.  The
kernel text is cut at labels, branches, barriers and s_endpgm; a K BLOCK is a block that holds MFMAs.  Each K block is walked on its own:
    vmcnt    every buffer_ / global_ load and store, in issue order: `s_waitcnt vmcnt(N)` completes all but the newest N.  What is in flight
             when the block is entered is older than everything the block issues, so a wait forces a load OF THE BLOCK exactly when fewer
             than N + 1 vector-memory instructions were issued behind it -- no knowledge of the entry state is needed.
For every buffer_load of a K block: the number of MFMAs between its issue and the first wait of the block that forces it (its COVER), or,
when the block ends first, OPEN with the MFMAs up to the block's end as a lower bound.  A block that branches back to its own label
(the K loop proper) is walked a second time to close what the first trip leaves open.
Loads are split by buffer descriptor as in wino_sched.py: the descriptor most loads of the K blocks go through is the weights', everything
else is an ACTIVATION load (the next chunk's patch; in the last chunk bias and residual pieces of the epilogue forms).
Per K block also the scalar loads in the text between the previous K block and its own end.  In the pipelined form (FORM 2) the first
four K blocks -- loop and three tails -- are the chunk that stages a successor, the last four the last chunk; FORM 1 has the last chunk only.
Per kernel: registers and scratch (.amdhsa), the K blocks, and over the SPAN of the text from the first K block to the last: scalar loads,
vmcnt(0) waits inside K blocks, and activation loads forced by a wait inside a K block.
usage: tools/conv_sched.py [--match "conv_igemm_f32<1, 3, 12, 1"] [--src other.hip] [--json out.json] [--quiet] [extra hipcc flags]
"""
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_sched as ws  # noqa: E402

CSRC = ws.CSRC


def kernel_blocks(asm):
    """-> {demangled kernel name: dict(blocks=[dict(label=, ins=[...])], vgpr=, scratch=)}"""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.Lfunc_end\d+:" % re.escape(sym), asm, flags=re.M | re.S)
        if not m:
            continue
        blocks, cur = [], dict(label=None, ins=[])
        for line in m.group(1).splitlines():
            lab = re.match(r"(\.LBB\d+_\d+):", line)
            if lab:
                if cur["ins"] or cur["label"]:
                    blocks.append(cur)
                cur = dict(label=lab.group(1), ins=[])
                continue
            t = " ".join(line.split(";")[0].split())
            if not t or t.endswith(":") or t.startswith("."):
                continue
            cur["ins"].append(t)
            if t.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_setpc")):
                blocks.append(cur)
                cur = dict(label=None, ins=[])
        if cur["ins"]:
            blocks.append(cur)
        hsa = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, flags=re.S).group(1)

        def field(name):
            f = re.search(r"\.amdhsa_%s\s+(\d+)" % name, hsa)
            return int(f.group(1)) if f else 0
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", dem)] = dict(
            blocks=blocks, vgpr=field("next_free_vgpr"), scratch=field("private_segment_fixed_size"))
    return out


def walk_block(ins, trips):
    """in-order vmcnt walk of one block, `trips` times over; -> (loads of the first trip, vmcnt(0) waits of the first trip)"""
    vm, loads, n_mfma, vm0 = [], [], 0, 0
    for trip in range(trips):
        for t in ins:
            if ws.is_mfma(t):
                n_mfma += 1
            elif ws.is_vmem(t):
                e = dict(op=t.split()[0], desc=ws.descriptor(t), at=n_mfma, cover=None, load="load" in t.split()[0], mine=trip == 0)
                vm.append(e)
                if e["load"] and trip == 0:
                    loads.append(e)
            elif t.startswith("s_waitcnt"):
                w = ws.wait_counts(t)
                if "vmcnt" in w:
                    vm0 += trip == 0 and w["vmcnt"] == 0
                    for e in vm[:max(len(vm) - w["vmcnt"], 0)]:
                        e["cover"] = n_mfma - e["at"]
                        e["forced_in_trip"] = trip
                    del vm[:max(len(vm) - w["vmcnt"], 0)]
    for e in vm:
        if e["mine"]:
            e["open_after"] = n_mfma - e["at"]  # (MFMAs up to the end of the walk: a lower bound of the cover)
    return loads, vm0


def analyse(k):
    blocks = k["blocks"]
    kidx = [i for i, b in enumerate(blocks) if any(ws.is_mfma(t) for t in b["ins"])]
    out = dict(vgpr=k["vgpr"], scratch=k["scratch"], k_blocks=[], span=None)
    if not kidx:
        return out
    counts = {}
    per = []
    for i in kidx:
        b = blocks[i]
        last = b["ins"][-1]
        loop = bool(b["label"]) and last.startswith("s_cbranch") and last.split()[-1] == b["label"]
        loads, vm0 = walk_block(b["ins"], 2 if loop else 1)
        for e in loads:
            counts[e["desc"]] = counts.get(e["desc"], 0) + 1
        per.append((b, loop, loads, vm0))
    # the weights' descriptor: what the K loop proper loads through (it fetches nothing else); a kernel without such a loop: the most used one
    loop_counts = {}
    for b, loop, loads, vm0 in per:
        for e in loads:
            if loop:
                loop_counts[e["desc"]] = loop_counts.get(e["desc"], 0) + 1
    wdesc = max(loop_counts, key=lambda d: loop_counts[d]) if loop_counts else (max(counts, key=lambda d: counts[d]) if counts else None)
    for (b, loop, loads, vm0), i, prev in zip(per, kidx, [None] + kidx[:-1]):
        rows = [dict(kind="weight" if e["desc"] == wdesc else "activation", issued_at_mfma=e["at"], cover=e["cover"],
                     open_after=e.get("open_after")) for e in loads]

        def least(kind):
            c = [r["cover"] if r["cover"] is not None else r["open_after"] for r in rows if r["kind"] == kind]
            return min(c) if c else None
        out["k_blocks"].append(dict(
            label=b["label"], loop=loop,
            smem_since_previous_k_block=0 if prev is None else sum(ws.is_smem(t) for bb in blocks[prev + 1:i + 1] for t in bb["ins"]),
            mfma=sum(ws.is_mfma(t) for t in b["ins"]), vmcnt0=vm0,
            n=dict(weight=sum(r["kind"] == "weight" for r in rows), activation=sum(r["kind"] == "activation" for r in rows)),
            least_cover=dict(weight=least("weight"), activation=least("activation")),
            activation_forced_in_block=sum(r["kind"] == "activation" and r["cover"] is not None for r in rows), loads=rows))
    span = blocks[kidx[0]:kidx[-1] + 1]
    out["weights_desc"] = wdesc
    out["span"] = dict(blocks=len(span), k_blocks=len(kidx), scalar_loads=sum(ws.is_smem(t) for b in span for t in b["ins"]),
                       vmcnt0_in_k_blocks=sum(kb["vmcnt0"] for kb in out["k_blocks"]),
                       activation_loads_forced_in_k_blocks=sum(kb["activation_forced_in_block"] for kb in out["k_blocks"]),
                       least_weight_cover=min([kb["least_cover"]["weight"] for kb in out["k_blocks"] if kb["least_cover"]["weight"] is not None], default=None))
    return out


def table(src=None, match="conv_igemm_f32", extra=(), only=None):
    """only: [(MT, NT, CAP, PF, FORM, EPI), ...] -- compile just these instantiations (seconds instead of minutes for the whole family)"""
    if only:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            tu = os.path.join(td, "conv_only.hip")
            with open(tu, "w") as f:
                f.write('#define I2R_CONV_KERNELS_ONLY\n#include "%s"\nnamespace {\n' % os.path.join(CSRC, "i2r_conv.hip"))
                for t in sorted(set(only)):
                    f.write("template __global__ void conv_igemm_f32<%d, %d, %d, %d, %d, %d>(const ConvGroupK);\n" % tuple(t))
                f.write("}\n")
            asm = ws.compile_asm(tu, extra)
    else:
        asm = ws.compile_asm(src or os.path.join(CSRC, "i2r_conv.hip"), extra)
    return {name: analyse(k) for name, k in sorted(kernel_blocks(asm).items()) if match in name}


def show(result):
    for name, k in result.items():
        s = k["span"]
        print("%s: %d VGPRs, scratch %d; K span: %d blocks (%d with MFMAs), %d scalar loads, %d vmcnt(0) in K blocks, %d activation loads forced "
              "in K blocks, least weight cover %s" % (name, k["vgpr"], k["scratch"], s["blocks"], s["k_blocks"], s["scalar_loads"],
                                                      s["vmcnt0_in_k_blocks"], s["activation_loads_forced_in_k_blocks"], s["least_weight_cover"]))
        for kb in k["k_blocks"]:
            print("  %-10s %s %3d MFMAs: weights %d (least cover %s), activations %d (least cover %s), vmcnt(0) %d" % (
                kb["label"], "loop" if kb["loop"] else "    ", kb["mfma"], kb["n"]["weight"], kb["least_cover"]["weight"], kb["n"]["activation"],
                kb["least_cover"]["activation"], kb["vmcnt0"]))


def main(argv):
    src, match, out_json, quiet, extra = None, "conv_igemm_f32", None, False, []
    it = iter(argv)
    for a in it:
        if a == "--src":
            src = next(it)
        elif a == "--match":
            match = next(it)
        elif a == "--json":
            out_json = next(it)
        elif a == "--quiet":
            quiet = True
        else:
            extra.append(a)
    result = table(src, match, extra)
    if not quiet:
        show(result)
    if out_json:
        for k in result.values():  # (the per-load rows stay out of the committed tables: 200 kernels)
            for kb in k["k_blocks"]:
                del kb["loads"]
        json.dump(result, open(out_json, "w"), indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
