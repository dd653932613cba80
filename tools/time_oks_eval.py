"""Time the device OKS evaluation on a COCO-val-shaped synthetic set: 5 000 images, about 6 400 gts, about 100 k detections before the
max_dets cut (what a detector with a low score threshold hands to COCOeval).  Prints the two kernels' times (device events around the
raw C-ABI calls), the whole caller.oks_eval call with the per-person-count groups, and the numpy restatement tests/_cocoeval_ref.py on
the same data on this machine's CPU.

    python tools/time_oks_eval.py [--images 5000] [--reps 5] [--no-cpu]

Needs the GPU; measures nothing that a test asserts."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import i2r_amd  # noqa: E402,F401
from i2r_amd import cabi, caller  # noqa: E402


def draw(n_img, seed=0, J=17):
    """-> gts, dts (lists of dicts as in the annotation / result file), image ids"""
    rng = np.random.default_rng(seed)
    gts, dts = [], []
    for img in range(1, n_img + 1):
        n_gt = int(rng.choice([1, 1, 1, 1, 1, 2, 2, 3, 4, 8])) if rng.uniform() < .54 else 0   # about 1.3 per image, half without
        poses = []
        for _ in range(n_gt):
            size = rng.uniform(30, 300)
            kp = np.zeros((J, 3))
            kp[:, :2] = np.round((rng.uniform(0, 600, 2) + rng.uniform(0, 1, (J, 2)) * size) * 256) / 256
            kp[:, 2] = rng.choice([0, 1, 2], J, p=[.2, .3, .5])
            lo, hi = kp[:, :2].min(0), kp[:, :2].max(0)
            gts.append(dict(image_id=img, keypoints=kp.reshape(-1).tolist(), area=float((hi - lo).prod() * .5),
                            bbox=[lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]], iscrowd=int(rng.uniform() < .02),
                            num_keypoints=int((kp[:, 2] > 0).sum())))
            poses.append(kp[:, :2])
        for _ in range(int(rng.integers(8, 33))):   # about 20 detections per image
            if poses and rng.uniform() < .6:
                xy = poses[rng.integers(0, len(poses))] + rng.standard_normal((J, 2)) * 10.0 ** rng.uniform(-1, 1.5)
            else:
                xy = rng.uniform(0, 600, 2) + rng.uniform(0, 1, (J, 2)) * rng.uniform(20, 300)
            kp = np.concatenate([np.round(xy * 256) / 256, np.ones((J, 1))], 1)
            dts.append(dict(image_id=img, keypoints=kp.reshape(-1).tolist(), score=float(np.float32(rng.uniform()))))
    return gts, dts, list(range(1, n_img + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    gts, dts, ids = draw(a.images)
    dev = torch.device("cuda", 0)
    anns = [dict(g, id=i + 1, category_id=1) for i, g in enumerate(gts)]
    gt = caller.GtTable.from_coco(dict(images=[dict(id=i) for i in ids], annotations=anns, categories=[dict(id=1, name="person")]))
    kp = torch.from_numpy(np.asarray([d["keypoints"] for d in dts], np.float32).reshape(len(dts), 17, 3)).to(dev)
    sc = torch.tensor([d["score"] for d in dts], dtype=torch.float32, device=dev)
    img = [d["image_id"] for d in dts]
    groups = caller.person_count_groups(gt.counts)
    print("%d images, %d gts, %d detections, groups %s + all" % (len(ids), len(gts), len(dts), groups[1]))

    # the whole call (host plumbing + two kernels + stats), and the kernels alone through a hook on the library
    L = cabi.lib()
    spans = {}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for name in ("i2r_oks_match", "i2r_oks_accumulate"):
        fn = getattr(L, name)

        def timed(args, stream, fn=fn, name=name):
            e0, e1 = ev(), ev()
            e0.record()
            rc = fn(args, stream)
            e1.record()
            spans.setdefault(name, []).append((e0, e1))
            return rc
        setattr(L, name, timed)
    walls = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = caller.oks_eval(gt, img, kp, sc, groups=groups)
        stats = res.stats.cpu()
        walls.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    for name, s in spans.items():
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in s[1:])
        print("%-20s median %.3f ms (min %.3f, max %.3f, %d runs)" % (name, ms[len(ms) // 2], ms[0], ms[-1], len(ms)))
    w = sorted(walls[1:])
    print("caller.oks_eval + stats on the host: median %.2f ms (min %.2f, max %.2f); first call %.2f ms" % (w[len(w) // 2] * 1e3, w[0] * 1e3, w[-1] * 1e3, walls[0] * 1e3))
    print("all:", [round(v, 4) for v in stats[-1].tolist()])
    if not a.no_cpu:
        import _cocoeval_ref as ref
        t0 = time.perf_counter()
        e = ref.run(gts, dts, ids)
        t1 = time.perf_counter()
        print("numpy restatement, every image (1 of the 5 evaluations of the per-person-count table): %.1f s; largest difference %.2e"
              % (t1 - t0, float(np.abs(e.stats - stats[-1].numpy()).max())))


if __name__ == "__main__":
    main()
