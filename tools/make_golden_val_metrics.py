"""Generate tests/golden/val_metrics_reference.npz by running THE REFERENCE ITSELF on CPU: JointsDataset.generate_target (called unbound
on a stand-in `self`, lib/dataset/JointsDataset.py:394-450), JointsMSELoss (lib/core/loss.py:15-41, both use_target_weight values) and
accuracy (lib/core/evaluate.py:41-71) -- the three calls behind the `Loss ... Accuracy ...` line of validate().
Run where the reference exists (oracle/ref_shim.py REF_ROOT):

    python tools/make_golden_val_metrics.py

cv2, pycocotools, crowdposetools, json_tricks, matplotlib, torchvision and the compiled NMS are stand-in modules: imported at module top
only, never called on this path.

Cases (S, J, h, w): (1, 1, 7, 5), (1, 17, 16, 12), (5, 17, 20, 20), (3, 14, 17, 13), (2, 14, 64, 48); sigma 2.  Joints are drawn over
[-9, w + 9] x [-9, h + 9], about 20 % invisible and 5 % with visibility 0.5 (not drawn, yet weighted); where a case holds at least 8
joints, 8 of them are planted on both sides of the four weight cut-offs (mu_x = -8 -> weight 0, -7.999 keeps it; mu_x = w + 6 -> 0,
w + 5.999 keeps it; the same in y).  output = target + N(0, 0.05) on a 2^-16 grid, the maps of one crop (of every second joint where
S == 1) rolled by 3 px in x and y, so that hits and misses both occur.  The (5, 17, 20, 20) case uses the COCO joints_weight table.
A joint is redrawn until (a) both fractional parts of mu lie >= 1e-3 from 0.5 (where rounding decides the target's arg-max); a case is
redrawn until (b) every dist that accuracy compares lies >= 1e-6 from 0.5.  The achieved minima, and the relative distance between the
reference's fp32 loss and the float64 sum of the same fp32 terms, are stored with every case.  Data only."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ref_shim import REF_LIB  # noqa: E402

CASES = [(1, 1, 7, 5), (1, 17, 16, 12), (5, 17, 20, 20), (3, 14, 17, 13), (2, 14, 64, 48)]
WEIGHTED_CASE = 2
SIGMA = 2
FRAC_MARGIN, DIST_MARGIN = 1e-3, 1e-6


def import_reference():
    def mod(name, **attrs):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
        return sys.modules[name]
    mod("nms.cpu_nms", cpu_nms=None)
    mod("nms.gpu_nms", gpu_nms=None)
    mod("pycocotools")
    mod("pycocotools.coco", COCO=None)
    mod("pycocotools.cocoeval", COCOeval=None)
    mod("crowdposetools")
    mod("crowdposetools.coco", COCO=None)
    mod("crowdposetools.cocoeval", COCOeval=None)
    mod("json_tricks")
    try:
        import scipy.io  # noqa: F401  (mpii.py, imported by the dataset package)
    except ImportError:
        mod("scipy")
        mod("scipy.io", loadmat=None, savemat=None)
    mod("cv2")
    mod("matplotlib")
    mod("matplotlib.pyplot")
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms")
    if not hasattr(np, "float"):
        np.float = float
    sys.path.insert(0, REF_LIB)
    from core.evaluate import accuracy, calc_dists
    from core.inference import get_max_preds
    from core.loss import JointsMSELoss
    from dataset.JointsDataset import JointsDataset
    return JointsDataset, JointsMSELoss, accuracy, calc_dists, get_max_preds


def frac_margin(mu):
    f = np.abs(mu - np.floor(mu) - 0.5)
    return float(f.min())


def draw_case(rng, S, J, h, w):
    """-> joints_hm float64 [S, J, 2], joints_vis fp32 [S, J], plants int32 [n, 2] (crop, joint), min frac margin"""
    mu = np.zeros((S, J, 2))
    for s in range(S):
        for j in range(J):
            while True:
                m = np.array([rng.uniform(-9, w + 9), rng.uniform(-9, h + 9)])
                if rng.random() < 0.6:   # most joints inside the map, so that counted joints are the rule
                    m = np.array([rng.uniform(0, w - 1), rng.uniform(0, h - 1)])
                if frac_margin(m) >= FRAC_MARGIN:
                    break
            mu[s, j] = m
    u = rng.random((S, J))
    vis = np.where(u < 0.2, 0.0, np.where(u < 0.25, 0.5, 1.0)).astype(np.float32)
    plants = np.zeros((0, 2), np.int32)
    if S * J >= 8:
        cx, cy = (w - 1) * 0.5 + 0.25, (h - 1) * 0.5 + 0.25
        pts = [(-8.0, cy), (-7.999, cy), (w + 6.0, cy), (w + 5.999, cy), (cx, -8.0), (cx, -7.999), (cx, h + 6.0), (cx, h + 5.999)]
        where = rng.permutation(S * J)[:8]
        plants = np.stack([where // J, where % J], 1).astype(np.int32)
        for (s, j), p in zip(plants, pts):
            mu[s, j] = p
            vis[s, j] = 1.0
    else:
        mu[0, 0] = [w * 0.5 + 0.3, h * 0.5 - 0.2]   # the single joint of the smallest case: drawn and counted
        vis[0, 0] = 1.0
    return mu, vis, plants, frac_margin(mu)


def main():
    import torch
    JointsDataset, JointsMSELoss, accuracy, calc_dists, get_max_preds = import_reference()
    coco_weight = np.array([1., 1., 1., 1., 1., 1., 1., 1.2, 1.2, 1.5, 1.5, 1., 1., 1.2, 1.2, 1.5, 1.5], np.float32)  # coco.py:106-112
    data = {"cases": np.asarray(CASES, np.int32), "sigma": np.int32(SIGMA), "numpy_version": np.asarray(np.__version__),
            "torch_version": np.asarray(torch.__version__), "frac_margin_required": np.float64(FRAC_MARGIN),
            "dist_margin_required": np.float64(DIST_MARGIN)}
    for ci, (S, J, h, w) in enumerate(CASES):
        jw = coco_weight if ci == WEIGHTED_CASE else None
        attempt = 0
        while True:
            rng = np.random.default_rng([ci, attempt])
            mu, vis, plants, fmargin = draw_case(rng, S, J, h, w)
            me = types.SimpleNamespace(num_joints=J, target_type="gaussian", heatmap_size=np.array([w, h]), sigma=SIGMA,
                                       use_different_joints_weight=jw is not None, joints_weight=None if jw is None else jw.reshape(J, 1))
            me.adjust_target_weight = lambda joint, tw, tmp: JointsDataset.adjust_target_weight(me, joint, tw, tmp)
            target, tweight = np.zeros((S, J, h, w), np.float32), np.zeros((S, J, 1), np.float32)
            for s in range(S):
                joints = np.concatenate([mu[s], np.zeros((J, 1))], 1)            # joints_3d is float64
                jv = np.stack([vis[s], vis[s], np.zeros(J, np.float32)], 1)
                target[s], tweight[s] = JointsDataset.generate_target(me, joints, jv)
            assert target.dtype == np.float32 and tweight.dtype == np.float32
            noise = rng.normal(0.0, 0.05, (S, J, h, w))
            moved = target.copy()
            if S == 1:
                moved[0, 1::2] = np.roll(target[0, 1::2], (3, 3), (1, 2))
            else:
                moved[S - 1] = np.roll(target[S - 1], (3, 3), (1, 2))
            output = (np.round((moved + noise) * 65536) / 65536).astype(np.float32)
            acc, avg_acc, cnt, pred = accuracy(output, target)
            tp, _ = get_max_preds(target)
            dists = calc_dists(pred, tp, np.ones((S, 2)) * np.array([h, w]) / 10)
            comp = dists[dists != -1]
            dmargin = float(np.abs(comp - 0.5).min()) if comp.size else np.inf
            if dmargin >= DIST_MARGIN:
                break
            attempt += 1
        q = "c%d_" % ci
        to, tt, tw_t = torch.from_numpy(output), torch.from_numpy(target), torch.from_numpy(tweight)
        for use_w in (1, 0):
            loss = JointsMSELoss(bool(use_w))(to, tt, tw_t, [S])
            assert loss.dtype == torch.float32
            wt = tw_t.reshape(S, J, 1) if use_w else None
            p, t = to.reshape(S, J, -1), tt.reshape(S, J, -1)
            d = (p.mul(wt) - t.mul(wt)) if use_w else (p - t)
            sse = (d * d).double().sum((0, 2))
            loss64 = float((0.5 * (sse / (S * h * w))).sum() / J)
            data[q + "loss_w%d" % use_w] = np.float32(loss.item())
            data[q + "loss64_w%d" % use_w] = np.float64(loss64)
            data[q + "loss_rel_w%d" % use_w] = np.float64(abs(float(loss.item()) - loss64) / loss64)
        data[q + "joints_hm"], data[q + "joints_vis"] = mu, vis
        data[q + "joints_weight"] = jw if jw is not None else np.zeros(0, np.float32)
        data[q + "output"], data[q + "target"], data[q + "target_weight"] = output, target, tweight.reshape(S, J)
        data[q + "acc"], data[q + "avg_acc"], data[q + "cnt"], data[q + "pred"] = acc, np.float64(avg_acc), np.int32(cnt), pred
        data[q + "plants"] = plants
        data[q + "min_frac_margin"], data[q + "min_dist_margin"], data[q + "redraws"] = np.float64(fmargin), np.float64(dmargin), np.int32(attempt)
        n_hit = int((comp < 0.5).sum())
        print("case %s: %d redraw(s), counted %d (hits %d), zero-weight %d, frac margin %.3g, dist margin %.3g, loss rel %.3g / %.3g"
              % ((S, J, h, w), attempt, comp.size, n_hit, int((tweight == 0).sum()), fmargin, dmargin, data[q + "loss_rel_w1"], data[q + "loss_rel_w0"]))
    path = os.path.join(ROOT, "tests", "golden", "val_metrics_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
