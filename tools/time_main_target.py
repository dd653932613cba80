"""GPU measurement: what sharing the first stage buys the grouped test mode ("Grouped inference").
Default: w48_pure_en6 fp32, 8 images x 4 persons, main-target groups of max_patch 3 and 5.  With --config (and --precision): that config at
its yaml's DATASET.MAX_PATCH (or --max-patch), images of as many persons as a full group has (max_patch, at least 4) -- the models with a
first stage of their own (TransPose-H, HRFormer), whose shared way is share_first_stage=True.  Three ways through the same engine,
alternated round by round, each timed with device events around a block of back-to-back calls that ends in a synchronise:

    plain      Engine.forward(x, pos_mask, length)                      the crops, every image one group (no grouping)
    expanded   Engine.forward(x[members], pos_mask[members], group_len)  every member of every group through the whole network: the
               path before the first stage was shared (forward_groups(share_first_stage=False) where --config is given); the gather of
               the inputs is timed with it (it is part of that path), first rows kept
    shared     Engine.forward_groups(x, pos_mask, members, group_len)    first stage once per person, tail on the gathered rows

Prints per max_patch the median, minimum and maximum of the rounds in ms per call, the ratios, the max-abs difference between the
shared and the expanded result and, for a shared program with i2r_rows_gather_multi launches, their in-situ durations (one timed replay
with a start marker in front of every launch); one JSON line per config at the end.
usage: python tools/time_main_target.py [--config NAME] [--precision fp32|bf16|fp16] [--max-patch P ...] [--images 8] [--rounds 7]
                                        [--calls 20] [--out FILE]   (--out: the JSON lines are APPENDED)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import i2r_amd  # noqa: E402,F401
from i2r_amd import arch, cabi, config, engine, synth  # noqa: E402
from i2r_amd import input as i2r_input  # noqa: E402


def multi_gather_us(eng, shared):
    """in-situ durations [us] of the i2r_rows_gather_multi launches of the shared program: one replay through i2r_run_program_timed"""
    engine.Program.timing_log = []
    try:
        shared()
        torch.cuda.synchronize()
        out = []
        for P, t0, t1, _ in engine.Program.timing_log:
            out += [round(1e3 * t0[i].elapsed_time(t1[i]), 2) for i, (kind, _, _) in enumerate(P.ops) if kind == cabi.GROUPS_OP_ROWS_GATHER_MULTI]
        return out
    finally:
        engine.Program.timing_log = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default=None, help="config name (default: w48_pure_en6 at max_patch 3 and 5)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--max-patch", type=int, nargs="*", default=None)
    ap.add_argument("--images", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cname = args.config or "w48_pure_en6"
    cfg = config.load_config(cname)
    patches = args.max_patch or ([3, 5] if args.config is None else [int(cfg.DATASET.MAX_PATCH)])
    sd = synth.make_state_dict(arch.param_spec(cfg))
    eng = engine.Engine(cfg, sd, dev, precision=args.precision)
    share = True if eng.singleformer else None  # (None: the HRNet-tower models share by default)
    length = [4 if args.config is None else max(4, max(patches))] * args.images
    W, H = cfg.MODEL.IMAGE_SIZE
    x, pm, _ = synth.make_inputs(length, H, W, 0)
    x, pm = x.to(dev), pm.to(dev)
    S = sum(length)
    # boxes: the persons of an image at seeded corners of a 640 x 480 frame
    u = synth.uniform01(5, "time_main_target.boxes", 2 * S).reshape(S, 2)
    boxes = torch.tensor(u * [560.0, 400.0], dtype=torch.float64)
    result = dict(workload=cname, precision=args.precision, share_first_stage=share, length=length, rounds=args.rounds, calls=args.calls, cases=[])
    for p in patches:
        groups = i2r_input.main_target_groups(boxes, length, p, dev)
        idx = groups.members.long()
        first = torch.tensor(eng._first_rows(groups.group_len), dtype=torch.long, device=dev)

        def plain():
            return eng.forward(x, pm, length)

        def expanded():
            if args.config is not None:
                return eng.forward_groups(x, pm, groups.members, groups.group_len, share_first_stage=False)
            return eng.forward(x.index_select(0, idx), pm.index_select(0, idx), groups.group_len).index_select(0, first)

        def shared():
            return eng.forward_groups(x, pm, groups.members, groups.group_len, share_first_stage=share)
        ways = [("plain", plain), ("expanded", expanded), ("shared", shared)]
        for _, fn in ways:  # warm up every shape the timed window uses (programs built, code objects loaded)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        err = (shared() - expanded()).abs().max().item()
        times = {name: [] for name, _ in ways}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, fn in ways:  # alternated: a drift of the machine hits all three alike
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.calls)
        med = {k: statistics.median(v) for k, v in times.items()}
        case = dict(max_patch=p, crops=S, expanded_crops=int(idx.numel()), groups=groups.n_groups, shared_vs_expanded_max_abs=err,
                    ms={k: dict(median=round(med[k], 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in times.items()},
                    expanded_over_shared=round(med["expanded"] / med["shared"], 3), shared_over_plain=round(med["shared"] / med["plain"], 3),
                    expanded_over_plain=round(med["expanded"] / med["plain"], 3), n_builds=eng.n_builds)
        gathers = multi_gather_us(eng, shared)
        if gathers:
            case["rows_gather_multi_us"] = gathers
        result["cases"].append(case)
        print("max_patch %d: %d crops -> %d expanded; ms per call (median [min, max] of %d rounds x %d calls)" % (p, S, idx.numel(), args.rounds, args.calls))
        for k in ("plain", "expanded", "shared"):
            print("    %-9s %8.3f  [%.3f, %.3f]" % (k, med[k], min(times[k]), max(times[k])))
        print("    expanded / shared %.2f   shared / plain %.2f   expanded / plain %.2f   shared vs expanded max-abs %.2e"
              % (case["expanded_over_shared"], case["shared_over_plain"], case["expanded_over_plain"], err))
        if gathers:
            print("    i2r_rows_gather_multi in situ: %s us (hand-over, first rows)" % ", ".join("%.1f" % t for t in gathers))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
