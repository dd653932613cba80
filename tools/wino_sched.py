#!/usr/bin/env python3
"""Static load / wait schedule of the Winograd kernels' pass loop (no GPU needed).

Compiles csrc/i2r_conv_wino.hip device-only to gfx950 assembly with the compile line of tools/wino_icount.py, splits every kernel at
the workgroup barriers like that tool (and at unconditional branches: a rotated loop has its closing barrier above its body), and walks the instruction list of each PASS region (a region that holds MFMAs) with an in-order
model of the two counters a wave waits on:
    vmcnt    every buffer_ / global_ load and store; they return in issue order, so `s_waitcnt vmcnt(N)` completes all but the newest N
    lgkmcnt  LDS operations (in order among themselves) and scalar loads (out of order: only lgkmcnt(0) completes them); the two
             are kept in queues of their own, as the hardware does, and a wait completes all but the newest N of the LDS queue
For every buffer_load of a region it gives the number of MFMAs between its issue and the first s_waitcnt that forces its completion
(its COVER), for every ds_read_b128 the same against lgkmcnt, and the number of `vmcnt(0)` waits, in the whole region and between
its first MFMA and its staging store (the first ds_write behind an MFMA; the end of the region where it has none).

Loads are split by buffer descriptor: the descriptor most loads of the region go through is the weights' (rs_w: 3 or 4 loads per
position against 2 per staging term), every other one an activation (rs_in, rs_t1, rs_t2, residuals).  The walk of a pass begins with what the
region before it leaves in flight (the set-up in front of a first pass, a further pass in front of a further or last one).  A load still outstanding at the
region's end is OPEN; its cover is then counted on into the region that runs next (a further pass after the first and after itself),
which is where the next pass's position-0 weights are waited for; an open load of a pass that no pass follows has no cover (null).

The walk is STATIC and in text order: a pass region holds the blocks of its `more` branch (the next chunk's staging), so it describes a
pass that another one follows.  Pass regions are named by what they hold:
    first    MFMAs with a literal zero as C and a staging store        further  neither zero C ... with a staging store
    only     zero C, no staging store (a one-pass item)                last     no zero C, no staging store
It looks at nothing but loads, LDS reads, waits and MFMAs.
usage: tools/wino_sched.py [--match "conv_wino_f32<1, 3"] [--src other.hip] [--json out.json] [--quiet] [extra hipcc flags]
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc")


def compile_asm(src, extra=()):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        s = os.path.join(td, "k.s")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-mllvm", "-amdgpu-mfma-vgpr-form",
                               "-I", os.path.join(ROOT, "include"), "-I", os.path.dirname(src), "-I", CSRC, "--cuda-device-only", "-S", src, "-o", s] + list(extra))
        return open(s).read()


def kernels(asm):
    """-> {demangled kernel name: dict(ins=[instruction text or '@loop', ...], vgpr=, agpr_offset=, scratch=)}"""
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M):
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.Lfunc_end\d+:" % re.escape(sym), asm, flags=re.M | re.S)
        if not m:
            continue
        ins = []
        for line in m.group(1).splitlines():
            if re.match(r"\.LBB\d+_\d+:.*This Loop Header: Depth=1", line) or ("@loop" not in ins and re.match(r"\.LBB\d+_\d+:.*in Loop: Header=\S+ Depth=1", line)):
                ins.append("@loop")  # (the loop over the fragments of a run, as in wino_icount.py)
            line = line.split(";")[0].strip()
            if not line or line.endswith(":") or line.startswith("."):
                continue
            ins.append(" ".join(line.split()))
        hsa = re.search(r"\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel" % re.escape(sym), asm, flags=re.S).group(1)

        def field(name, default=0):
            f = re.search(r"\.amdhsa_%s\s+(\d+)" % name, hsa)
            return int(f.group(1)) if f else default
        dem = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(anonymous namespace\)::|\(.*\)$|^void ", "", dem)] = dict(
            ins=ins, vgpr=field("next_free_vgpr"), accum_offset=field("accum_offset"), scratch=field("private_segment_fixed_size"))
    return out


def split_regions(ins):
    regs, cur = [], []
    for t in ins:
        if t != "@loop":
            cur.append(t)
        if t.startswith(("s_barrier", "s_branch", "s_endpgm", "s_setpc")) or t == "@loop":  # (what follows an unconditional branch in the text does not run next)
            regs.append(cur)
            cur = []
    regs.append(cur)
    return regs


def is_mfma(t):
    return t.startswith(("v_mfma", "v_smfma"))


def is_vmem(t):
    return t.startswith(("buffer_", "global_", "flat_", "scratch_")) and not t.startswith(("buffer_wbl2", "buffer_inv", "buffer_wbinvl1"))


def is_lds(t):
    return t.startswith("ds_")


def is_smem(t):
    return t.startswith(("s_load", "s_buffer_load"))


def descriptor(t):
    m = re.search(r"\b(s\[\d+:\d+\])", t)
    return m.group(1) if m else "-"


def wait_counts(t):
    """s_waitcnt text -> {counter: N} of the counters it names"""
    return {k: int(v) for k, v in re.findall(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)", t)}


class Walk:
    """in-order counters over one or more regions; entries are dicts shared with the result table"""

    def __init__(self):
        self.vm, self.lds, self.sm, self.n_mfma = [], [], [], 0

    def run(self, region, record):
        """walks `region`; record=True: its loads / reads enter the table (returned); False: only outstanding entries are completed"""
        loads, reads, vm0, vm0_pass = [], [], 0, 0
        first_mfma = next((i for i, t in enumerate(region) if is_mfma(t)), len(region))
        store_at = next((i for i, t in enumerate(region) if i > first_mfma and t.startswith("ds_write")), len(region))
        for i, t in enumerate(region):
            if is_mfma(t):
                self.n_mfma += 1
            elif is_vmem(t):
                e = dict(op=t.split()[0], desc=descriptor(t), at=self.n_mfma, cover=None, open=True, wrapped=False, load="load" in t.split()[0], own=record)
                self.vm.append(e)
                if record and e["load"]:
                    loads.append(e)
            elif is_lds(t):
                e = dict(op=t.split()[0], at=self.n_mfma, cover=None, open=True, wrapped=False, own=record)
                self.lds.append(e)
                if record and e["op"] == "ds_read_b128":
                    reads.append(e)
            elif is_smem(t):
                self.sm.append(t)
            elif t.startswith("s_waitcnt"):
                w = wait_counts(t)
                if "vmcnt" in w:
                    if record and w["vmcnt"] == 0:
                        vm0 += 1
                        vm0_pass += first_mfma < i < store_at
                    self._complete(self.vm, w["vmcnt"], record)
                if "lgkmcnt" in w:
                    if w["lgkmcnt"] == 0:
                        self.sm = []
                    self._complete(self.lds, w["lgkmcnt"], record)
        return loads, reads, vm0, vm0_pass

    def _complete(self, q, keep, record):
        done = q[:max(len(q) - keep, 0)]
        del q[:len(done)]
        for e in done:
            e["cover"] = self.n_mfma - e["at"]
            e["wrapped"] = not (record and e["own"])
            if record and e["own"]:
                e["open"] = False


def pass_kind(region):
    zero_c = any(is_mfma(t) and t.rstrip().endswith(", 0") for t in region)
    first_mfma = next(i for i, t in enumerate(region) if is_mfma(t))
    store = any(t.startswith("ds_write") for t in region[first_mfma:])
    return {(True, True): "first", (True, False): "only", (False, True): "further", (False, False): "last"}[(zero_c, store)]


def analyse(k):
    """kernel dict of kernels() -> {vgpr, scratch, regions: {kind: table}}"""
    passes, before = {}, {}
    regs = split_regions(k["ins"])
    for i, r in enumerate(regs):
        if any(is_mfma(t) for t in r):
            kind = pass_kind(r)
            while kind in passes:
                kind += "+"
            passes[kind] = r
            before[kind] = [b for b in regs[:i] if b and not any(is_mfma(t) for t in b)][-2:]  # (fragment set-up and the staging store of chunk 0: what a first pass finds in flight)
    out = dict(vgpr=k["vgpr"], accum_offset=k["accum_offset"], scratch=k["scratch"], regions={})
    for kind, r in passes.items():
        w = Walk()
        # what is in flight when the pass begins: the position-0 weights, fetched by the set-up or by the pass before
        if kind.startswith(("first", "only")):
            for b in before[kind]:
                w.run([t for t in b if not is_mfma(t)], False)
        else:
            w.run(passes.get("further", passes.get("first", r)), False)
        w.n_mfma = 0
        for e in w.vm + w.lds:
            e["at"] = 0
        loads, reads, vm0, vm0_pass = w.run(r, True)
        if kind in ("first", "further") and "further" in passes:  # (what is open is waited for in the pass that follows)
            w.run(passes["further"], False)
        counts = {}
        for e in loads:
            counts[e["desc"]] = counts.get(e["desc"], 0) + 1
        wdesc = max(counts, key=lambda d: counts[d]) if counts else None

        def row(e, kind_of=None):
            d = dict(op=e["op"], issued_at_mfma=e["at"], cover=e["cover"], open=e["open"])
            if kind_of:
                d.update(desc=e["desc"], kind=kind_of)
            return d
        lt = [row(e, "weight" if e["desc"] == wdesc else "activation") for e in loads]
        rt = [row(e) for e in reads]

        def least(rows):
            c = [x["cover"] for x in rows]
            return None if not c or any(v is None for v in c) else min(c)
        out["regions"][kind] = dict(
            mfma=sum(is_mfma(t) for t in r), vmcnt0=vm0, vmcnt0_before_staging_store=vm0_pass, weights_desc=wdesc,
            min_cover=dict(weight=least([x for x in lt if x["kind"] == "weight"]), activation=least([x for x in lt if x["kind"] == "activation"]),
                           ds_read_b128=least(rt)),
            n=dict(weight=sum(x["kind"] == "weight" for x in lt), activation=sum(x["kind"] == "activation" for x in lt), ds_read_b128=len(rt)),
            loads=lt, ds_reads=rt)
    return out


def table(src=None, match="conv_wino", extra=()):
    asm = compile_asm(src or os.path.join(CSRC, "i2r_conv_wino.hip"), extra)
    return {name: analyse(k) for name, k in sorted(kernels(asm).items()) if match in name}


def show(result):
    for name, k in result.items():
        print("%s: %d VGPRs, scratch %d" % (name, k["vgpr"], k["scratch"]))
        for kind, r in k["regions"].items():
            print("  %-8s %2d MFMAs, vmcnt(0) waits: %d (%d between the first MFMA and the staging store)" % (kind, r["mfma"], r["vmcnt0"], r["vmcnt0_before_staging_store"]))
            for what in ("weight", "activation"):
                rows = [x for x in r["loads"] if x["kind"] == what]
                print("    %-10s loads, issued@MFMA:cover  " % what + " ".join(
                    "%d:%s%s" % (x["issued_at_mfma"], "-" if x["cover"] is None else x["cover"], "(open)" if x["open"] else "") for x in rows))
            print("    ds_read_b128      issued@MFMA:cover  " + " ".join(
                "%d:%s%s" % (x["issued_at_mfma"], "-" if x["cover"] is None else x["cover"], "(open)" if x["open"] else "") for x in r["ds_reads"]))


def main(argv):
    src, match, out_json, quiet, extra = None, "conv_wino", None, False, []
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
        json.dump(result, open(out_json, "w"), indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
