"""GPU measurement aid for i2r_pose_nms (rescoring + OKS-NMS on the device).  Three modes:

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_pose_nms.py kernel      # the launches, in a profiler run of their own
    python tools/time_pose_nms.py parse DIR > profiles/pose_nms.json                     # per-shape kernel time out of DIR's kernel trace
    python tools/time_pose_nms.py pipeline                                                # the pipeline step with and without the NMS call

kernel: per shape REPS launches of the hard form, then REPS of the soft form, in the order of SHAPES (parse relies on that order); it also
prints what the kernel replaces, on the same inputs: the copy of the key points to the host + the numpy loops (tests/_nms_ref.py).
  config-1 shape 8 images x 4 persons | CrowdPose shape 57 crops (19 images x 3) | crowded batch 32 x 30 | one image of 200 persons
pipeline: bench.py's --pipeline step (uint8 image -> crops + masks -> flip-test forward -> key points, 8 x 4 persons, w48 fp32), driven from
here, ROUNDS rounds of alternating blocks of STEPS steps with and without caller.rescore_nms behind the decode; wall time per step."""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("config1_8x4", [4] * 8, 14), ("crowdpose_57", [3] * 19, 14), ("crowded_32x30", [30] * 32, 17), ("one_image_200", [200], 17)]
REPS = 20


def draw(length, J, seed):
    """clusters of three persons around shared base poses, jitter 0.05 .. 100 px (as tools/make_golden_nms.py draws them)"""
    rng = np.random.default_rng(seed)
    out = []
    for P in length:
        n_cl = max(1, -(-P // 3))
        base = rng.uniform(100, 900, (n_cl, 1, 2)) + rng.uniform(-60, 60, (n_cl, J, 2))
        cl = rng.integers(0, n_cl, P)
        mag = 10.0 ** rng.uniform(np.log10(0.05), 2.0, (P, 1, 1))
        out.append(base[cl] + mag * rng.standard_normal((P, J, 2)))
    S = sum(length)
    f = np.float32
    return (np.concatenate(out).astype(f), rng.uniform(0.05, 1, (S, J, 1)).astype(f), rng.uniform(0.8, 2.0, (S, 2)).astype(f),
            rng.uniform(0.3, 1, S).astype(f))


def kernel():
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import caller
    import _nms_ref
    for name, length, J in SHAPES:
        preds, maxv, scale, box = draw(length, J, 1)
        dp, dm, ds, db = (torch.from_numpy(a).cuda() for a in (preds, maxv, scale, box))
        row = dict(shape=name, images=len(length), crops=sum(length), joints=J)
        for soft in (False, True):
            caller.rescore_nms(dp, dm, ds, db, length, 0.2, 0.9, soft=soft)   # (first launch: code object load)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                got = caller.rescore_nms(dp, dm, ds, db, length, 0.2, 0.9, soft=soft)
            e1.record()
            torch.cuda.synchronize()
            row["soft" if soft else "hard"] = dict(call_us_event_timed=round(e0.elapsed_time(e1) / REPS * 1e3, 1), kept=int(got.n_keep.sum()))
            # what it replaces: key points to the host + the reference's loops
            t0 = time.perf_counter()
            hp, hm = dp.cpu().numpy(), dm.cpu().numpy()
            t1 = time.perf_counter()
            want = _nms_ref.run_batch(hp, hm, np.prod(scale * 200, 1), box, length, caller.SIGMAS[J], 0.2, 0.9, soft=soft)
            t2 = time.perf_counter()
            row["soft" if soft else "hard"].update(host_copy_us=round((t1 - t0) * 1e6, 1), host_numpy_us=round((t2 - t1) * 1e6, 1),
                                                   # (these inputs are not margin-filtered: informative only)
                                                   rank_equal_to_numpy=bool(np.array_equal(want[1], got.rank.cpu().numpy())))
        print(json.dumps(row), flush=True)


def parse(d):
    import csv
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for r in csv.DictReader(open(trace)) if "pose_nms_k" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    per = 2 * (REPS + 1)
    assert len(us) == per * len(SHAPES), (len(us), per * len(SHAPES))
    out = {}
    for k, (name, length, J) in enumerate(SHAPES):
        blk = us[k * per:(k + 1) * per]
        hard, soft = blk[1:REPS + 1], blk[REPS + 2:]
        out[name] = dict(images=len(length), crops=sum(length), joints=J,
                         hard_us=dict(median=round(float(np.median(hard)), 2), min=round(min(hard), 2), max=round(max(hard), 2)),
                         soft_us=dict(median=round(float(np.median(soft)), 2), min=round(min(soft), 2), max=round(max(soft), 2)))
    print(json.dumps(dict(what="i2r_pose_nms kernel time per launch, rocprofv3 --kernel-trace, %d launches per shape and form" % REPS, shapes=out), indent=1))


def pipeline():
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import arch, caller, config, models, synth
    import bench
    STEPS, ROUNDS = 20, 5
    dev = torch.device("cuda", 0)
    cfg = config.load_config("w48_pure_en6")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(synth.make_state_dict(arch.param_spec(cfg)), strict=True)
    net = net.to(dev)
    length = [4] * 8
    step = bench.make_pipeline(net, cfg, length, 256, 192, dev, seed=0)
    S = sum(length)
    scale = torch.full((S, 2), 1.3, device=dev)
    box = torch.linspace(0.5, 1.0, S, device=dev)

    def with_nms():
        preds, maxv = step()
        return caller.rescore_nms(preds, maxv, scale, box, length, 0.2, 0.9)

    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3
    for fn in (step, with_nms):
        for _ in range(5):
            fn()
    plain, nms = [], []
    for _ in range(ROUNDS):
        plain.append(block(step))
        nms.append(block(with_nms))
    print(json.dumps(dict(what="pipeline step (8 images x 4 persons, w48 fp32, flip test), ms per step, %d rounds of %d steps, alternating" % (ROUNDS, STEPS),
                          plain_ms=[round(v, 3) for v in plain], with_nms_ms=[round(v, 3) for v in nms],
                          plain_median=round(float(np.median(plain)), 3), with_nms_median=round(float(np.median(nms)), 3),
                          plain_spread=round(max(plain) - min(plain), 3), difference=round(float(np.median(nms) - np.median(plain)), 3))))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "parse":
        parse(sys.argv[2])
    else:
        {"kernel": kernel, "pipeline": pipeline}[mode]()
