"""GPU measurement aid for i2r_val_metrics / i2r_joint_targets (validation loss + PCK accuracy on the device).  Two modes:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_val_metrics.py kernel   # in a profiler run of its own
    python tools/time_val_metrics.py parse DIR > profiles/val_metrics.json                # per-shape kernel time out of DIR's kernel trace

kernel: per shape, in the order of SHAPES and BLOCKS (parse relies on that order): 1 + REPS launches in tensor mode on ONE batch (the
maps stay in the caches between launches), 1 + REPS in analytic mode on one batch, then the same two with every launch on a batch of its
own out of a ring of more than 512 MB (the maps come from HBM, as they do behind a forward), then 1 + REPS of i2r_joint_targets with
the target written.  It also prints what the kernels replace on the same inputs, shaped like the reference's loop body: the copy of
the heat maps to the host + the target upload + the numpy path (tests/_val_ref.py).
  config 1: 8 x 4 crops, 14 joints, 64 x 48 | config 3: 57 crops, 14 joints, 64 x 48 | 12 crops, 17 joints, 96 x 72"""
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("config1_32x14_64x48", 32, 14, 64, 48), ("config3_57x14_64x48", 57, 14, 64, 48), ("hrt288_12x17_96x72", 12, 17, 96, 72)]
BLOCKS = ("tensor_warm", "analytic_warm", "tensor_cold", "analytic_cold")
REPS = 20
RING_BYTES = 512 << 20     # more than the 256 MB of the last-level cache


def draw(S, J, h, w, seed):
    rng = np.random.default_rng(seed)
    mu = np.stack([rng.uniform(-9, w + 9, (S, J)), rng.uniform(-9, h + 9, (S, J))], 2)
    vis = (rng.random((S, J)) > 0.2).astype(np.float32)
    return mu, vis


def kernel():
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import caller
    import _val_ref
    dev = torch.device("cuda", 0)
    for name, S, J, h, w in SHAPES:
        mu, vis = draw(S, J, h, w, 1)
        hm, dv = torch.from_numpy(mu).to(dev), torch.from_numpy(vis).to(dev)
        target, tw = caller.joint_targets(hm, dv, (w, h))
        map_bytes = S * J * h * w * 4
        n_ring = -(-RING_BYTES // (2 * map_bytes))
        ring_t = target.unsqueeze(0).repeat(n_ring, 1, 1, 1, 1)
        ring_o = ring_t + 0.05 * torch.randn(ring_t.shape, device=dev, generator=torch.Generator(dev).manual_seed(2))
        row = dict(shape=name, crops=S, joints=J, h=h, w=w, map_bytes=map_bytes, ring_batches=n_ring)

        def launch(block, k):
            i = (k % n_ring) if block.endswith("cold") else 0
            if block.startswith("tensor"):
                return caller.val_metrics(ring_o[i], ring_t[i], tw)
            return caller.val_metrics(ring_o[i], joints_hm=hm, joints_vis=dv)
        for block in BLOCKS:
            launch(block, REPS)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(REPS):
                got = launch(block, k)
            e1.record()
            torch.cuda.synchronize()
            row[block] = dict(call_us_event_timed=round(e0.elapsed_time(e1) / REPS * 1e3, 1), loss=got.loss.item(), avg_acc=got.avg_acc.item())
        for _ in range(REPS + 1):
            caller.joint_targets(hm, dv, (w, h))
        torch.cuda.synchronize()
        # what it replaces: heat maps to the host, the target up, the reference-shaped numpy path
        th, twh = target.cpu(), tw.cpu()
        _val_ref.val_metrics(ring_o[0, :1].cpu().numpy(), th[:1].numpy(), twh[:1].numpy())   # (first call: numpy's own set-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ring_o[0].cpu().numpy()
        t1 = time.perf_counter()
        th.to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        want = _val_ref.val_metrics(out, th.numpy(), twh.numpy())
        t3 = time.perf_counter()
        got = caller.val_metrics(ring_o[0], ring_t[0], tw)
        row["host_path"] = dict(d2h_copy_us=round((t1 - t0) * 1e6, 1), target_upload_us=round((t2 - t1) * 1e6, 1), numpy_us=round((t3 - t2) * 1e6, 1),
                                total_us=round((t3 - t0) * 1e6, 1), loss_rel_diff_to_device=abs(want.loss - got.loss.item()) / want.loss,
                                acc_equal_to_device=bool(np.array_equal(want.acc, got.acc.cpu().numpy())))
        print(json.dumps(row), flush=True)
        del ring_o, ring_t


def parse(d):
    import csv
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))

    def times(tag):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if tag in r["Kernel_Name"]]

    def stat(v):
        return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2))
    maps = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if "val_metrics_map_k" in r["Kernel_Name"]]
    fin, jt = times("val_metrics_finish_k"), times("joint_targets_k")
    per = REPS + 1
    n_maps = len(BLOCKS) * per + 1          # (+ the comparison launch behind the host path)
    assert len(maps) == n_maps * len(SHAPES) == len(fin), (len(maps), len(fin))
    assert len(jt) == (per + 1) * len(SHAPES), len(jt)
    out = {}
    for k, (name, S, J, h, w) in enumerate(SHAPES):
        e = dict(crops=S, joints=J, h=h, w=w, map_bytes=S * J * h * w * 4)
        for b, block in enumerate(BLOCKS):
            blk = maps[k * n_maps + b * per:k * n_maps + (b + 1) * per]
            assert all(("<true>" in n) == block.startswith("analytic") for n, _ in blk), block
            us = [t for _, t in blk[1:]]
            e[block + "_us"] = stat(us)
            read = e["map_bytes"] * (2 if block.startswith("tensor") else 1)
            e[block + "_tb_per_s"] = round(read / (float(np.median(us)) * 1e-6) / 1e12, 3)
        e["finish_us"] = stat(fin[k * n_maps:(k + 1) * n_maps])
        e["joint_targets_us"] = stat(jt[k * (per + 1) + 2:(k + 1) * (per + 1)])
        out[name] = e
    print(json.dumps(dict(what="i2r_val_metrics kernel time per launch (val_metrics_map_k; val_metrics_finish_k follows every one), rocprofv3 "
                               "--kernel-trace, %d launches per shape and block; warm = one batch again and again, cold = a ring of batches "
                               "larger than the last-level cache; tb_per_s = bytes of maps read / median time" % REPS, shapes=out), indent=1))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "parse":
        parse(sys.argv[2])
    else:
        kernel()
