"""Generate tests/golden/nms_reference.npz by running THE REFERENCE ITSELF on CPU: the rescoring loop of its dataset class
(lib/dataset/coco.py COCODataset.evaluate for J = 17, crowdpose.py CROWDPOSEDataset.evaluate for J = 14, called unbound on a stand-in
`self`) and its own oks_nms / soft_oks_nms (lib/nms/nms.py).
Run where the reference exists (oracle/ref_shim.py REF_ROOT):

    python tools/make_golden_nms.py

The compiled box NMS (nms.cpu_nms / nms.gpu_nms, dead in the reference), pycocotools, crowdposetools, json_tricks, cv2, matplotlib and torchvision are
stand-in modules: they are imported at module top only and never called on this path.  evaluate() runs with image_set = 'test' (no
COCOeval) and a `_write_coco_keypoint_results` that keeps the lists it is handed instead of writing json.

Inputs: persons in clusters around shared base poses with jitter from 0.05 px to 100 px (both kept and suppressed persons), key points
on a 1/256 px grid, J = 17 and 14, images of 0, 1, 2 ... 40, 64, 100 and 200 persons.  ONE draw per joint count serves all four
(oks_thre, in_vis_thre) combinations.  An image is redrawn until, for every combination,
  (a) every OKS the reference compares with the threshold lies >= 1e-4 from it (recorded from its own oks_iou),
  (b) no two rescored scores of the image are equal as float32,
  (c) soft form: at every step the top decayed score exceeds the runner-up by a relative 1e-4 (recorded from its own rescore),
  (d) at most one person has no joint above in_vis_thre.
(e) "every set holds kept and suppressed persons" is asserted at the end.  The achieved minima are stored with every set.  Data only."""
import ast
import inspect
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from ref_shim import REF_LIB  # noqa: E402

COUNTS = list(range(41)) + [64, 100, 200]
COMBOS = [(0.9, 0.2), (0.9, 0.0), (0.5, 0.2), (0.5, 0.0)]  # (TEST.OKS_THRE, TEST.IN_VIS_THRE)
OKS_MARGIN, SOFT_GAP = 1e-4, 1e-4


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
    from nms import nms as ref_nms
    try:
        from dataset.coco import COCODataset
        from dataset.crowdpose import CROWDPOSEDataset
        COCODataset = {17: COCODataset, 14: CROWDPOSEDataset}  # (crowdpose.py hands num_joints on to the NMS, coco.py leaves 17)
    except Exception as e:  # noqa: BLE001
        print("dataset.coco does not import here (%r): rescoring will be restated" % (e,))
        COCODataset = None
    return ref_nms, COCODataset


def sigma_tables(ref_nms):
    """the two literal tables of oks_iou (nms.py:79-81), evaluated as the reference writes them: {J: float64 [J]}"""
    out = {}
    for node in ast.walk(ast.parse(inspect.getsource(ref_nms.oks_iou))):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") == "sigmas":
            v = eval(compile(ast.Expression(node.value), "<sigmas>", "eval"), {"np": np})
            out[len(v)] = np.asarray(v, np.float64)
    assert sorted(out) == [14, 17], sorted(out)
    return out


def draw_image(rng, P, J, lone_invisible):
    """-> preds [P, J, 2], maxvals [P, J], center [P, 2], scale [P, 2], box_score [P] (all float32)"""
    n_cl = max(1, int(np.ceil(P / 3.0)))
    base = rng.uniform(100, 900, (n_cl, 1, 2)) + rng.uniform(-60, 60, (n_cl, J, 2))
    cl_scale = rng.uniform(0.8, 2.0, (n_cl, 2))
    cl = rng.integers(0, n_cl, P)
    mag = 10.0 ** rng.uniform(np.log10(0.05), 2.0, (P, 1, 1))
    first = np.zeros(P, bool)  # the first member of a cluster sits on the base pose
    first[[int(np.argmax(cl == c)) for c in set(cl.tolist())]] = True
    mag[first] = 0.0
    preds = np.round((base[cl] + mag * rng.standard_normal((P, J, 2))) * 256) / 256
    maxvals = np.round(rng.uniform(0.05, 1.0, (P, J)) * 65536) / 65536
    if lone_invisible and P >= 3:
        maxvals[1] = np.round(rng.uniform(0.01, 0.19, J) * 65536) / 65536
    scale = cl_scale[cl] * rng.uniform(0.95, 1.05, (P, 2))
    center = np.round(rng.uniform(50, 950, (P, 2)) * 16) / 16
    box = rng.uniform(0.3, 1.0, P)
    f = np.float32
    return preds.astype(f), maxvals.astype(f), center.astype(f), scale.astype(f), box.astype(f)


class Recorder:
    """wraps the reference's oks_iou / rescore: calls them, keeps what they return"""

    def __init__(self, ref_nms):
        self.ref, self.oks, self.decayed = ref_nms, [], []
        self._oks_iou, self._rescore = ref_nms.oks_iou, ref_nms.rescore
        ref_nms.oks_iou, ref_nms.rescore = self.oks_iou, self.rescore

    def oks_iou(self, *a, **k):
        out = self._oks_iou(*a, **k)
        self.oks.append(np.array(out))
        return out

    def rescore(self, *a, **k):
        out = self._rescore(*a, **k)
        self.decayed.append(np.array(out))
        return out

    def reset(self):
        self.oks, self.decayed = [], []


def rescoring_restated(kp, box_score, in_vis_thre):
    """coco.py:384-396 on float32 numpy scalars (only used when the dataset class cannot be imported)"""
    out = []
    for p in range(kp.shape[0]):
        kpt_score, valid_num = 0, 0
        for j in range(kp.shape[1]):
            t_s = kp[p][j][2]
            if t_s > in_vis_thre:
                kpt_score = kpt_score + t_s
                valid_num = valid_num + 1
        if valid_num != 0:
            kpt_score = kpt_score / valid_num
        out.append(kpt_score * box_score[p])
    return out


def reference_image(ref_nms, COCODataset, rec, kp, center, scale, area, box, J, oks_thre, in_vis_thre):
    """One image through the reference: -> (scores float64 [P], keep_hard, keep_soft, min |oks - thr|, min soft gap)."""
    P = kp.shape[0]
    COCODataset = COCODataset[J] if COCODataset is not None else None
    boxes = np.zeros((P, 6))  # validate()'s all_boxes (function.py:218-221): a float64 container
    boxes[:, 0:2], boxes[:, 2:4], boxes[:, 4], boxes[:, 5] = center, scale, area, box
    out = {}
    for soft in (False, True):
        rec.reset()
        if COCODataset is not None:
            got = []
            me = types.SimpleNamespace(num_joints=J, in_vis_thre=in_vis_thre, oks_thre=oks_thre, soft_nms=soft, image_set="test",
                                       _write_coco_keypoint_results=lambda kpts, res_file: got.append(kpts),
                                       _do_python_keypoint_eval=lambda res_file, res_folder: [("AP", 0.0)])  # (crowdpose.py calls it always)
            with tempfile.TemporaryDirectory() as td:
                COCODataset.evaluate(me, types.SimpleNamespace(RANK=0), kp.copy(), td, boxes, ["%012d.jpg" % 7] * P)
            (img_kpts,) = got[0]
            where = {tuple(np.asarray(c, np.float64)): i for i, c in enumerate(center)}
            assert len(where) == P
            keep = [where[tuple(np.asarray(k["center"], np.float64))] for k in img_kpts]
            if not soft:
                # evaluate() leaves the rescored value in every person's dict; the suppressed ones are not handed on, so the scores
                # of ALL persons are read from a threshold-1.0 hard run, which keeps everyone (the score does not depend on the NMS)
                me_all = types.SimpleNamespace(**{**me.__dict__, "oks_thre": 1.0})
                hold = rec.oks, rec.decayed
                rec.reset()
                with tempfile.TemporaryDirectory() as td:
                    COCODataset.evaluate(me_all, types.SimpleNamespace(RANK=0), kp.copy(), td, boxes, ["%012d.jpg" % 7] * P)
                rec.oks, rec.decayed = hold
                (everyone,) = got[1]
                assert len(everyone) == P
                scores = np.zeros(P)
                for k in everyone:
                    scores[where[tuple(np.asarray(k["center"], np.float64))]] = k["score"]
        else:
            if not soft:
                scores = np.asarray(rescoring_restated(kp, boxes[:, 5], in_vis_thre), np.float64)
            db = [dict(keypoints=kp[i], area=boxes[i][4], score=scores[i]) for i in range(P)]
            keep = list((ref_nms.soft_oks_nms if soft else ref_nms.oks_nms)(db, oks_thre))
        out[soft] = [int(k) for k in keep]
        if not soft:
            margin = min([float(np.abs(o - oks_thre).min()) for o in rec.oks if o.size] or [np.inf])
        else:
            gap = np.inf
            top2 = [np.sort(scores)[::-1][:2]] + [np.sort(d)[::-1][:2] for d in rec.decayed]
            for step, t in enumerate(top2[:len(keep)]):  # the order BEFORE each pick decides it
                if t.size == 2:
                    gap = min(gap, (t[0] - t[1]) / t[0] if t[0] > 0 else 0.0)
    return scores, out[False], out[True], margin, gap


def main():
    ref_nms, COCODataset = import_reference()
    sig = sigma_tables(ref_nms)
    rec = Recorder(ref_nms)
    data = {"counts": np.asarray(COUNTS, np.int32), "combos": np.asarray(COMBOS, np.float64), "max_dets": np.int32(20),
            "rescoring_from_evaluate": np.bool_(COCODataset is not None), "oks_margin_required": np.float64(OKS_MARGIN),
            "soft_gap_required": np.float64(SOFT_GAP), "numpy_version": np.asarray(np.__version__)}
    for J in (17, 14):
        cols = {k: [] for k in ("preds", "maxvals", "center", "scale", "area", "box_score")}
        per = {c: dict(score=[], keep_hard=[], keep_soft=[], margin=np.inf, gap=np.inf, score_gap=np.inf, zero_max=0) for c in COMBOS}
        redraws = 0
        for n_i, P in enumerate(COUNTS):
            attempt = 0
            while True:
                rng = np.random.default_rng([J, P, attempt])
                preds, maxvals, center, scale, box = draw_image(rng, P, J, lone_invisible=(n_i % 5 == 3))
                area = np.prod(scale * 200, 1)  # function.py:220 on the loader's float32 scale
                assert area.dtype == np.float32
                kp = np.concatenate([preds, maxvals[:, :, None]], 2)
                res, ok = {}, True
                for thr, vis in COMBOS:
                    if P == 0:
                        res[(thr, vis)] = (np.zeros(0), [], [], np.inf, np.inf, np.inf, 0)
                        continue
                    scores, kh, ks, margin, gap = reference_image(ref_nms, COCODataset, rec, kp, center, scale, area, box, J, thr, vis)
                    s32 = np.sort(scores.astype(np.float32))
                    sgap = float(np.diff(s32).min()) if P > 1 else np.inf
                    n_zero = int(((maxvals > np.float32(vis)).sum(1) == 0).sum())
                    ok = ok and margin >= OKS_MARGIN and gap >= SOFT_GAP and sgap > 0 and n_zero <= 1
                    res[(thr, vis)] = (scores, kh, ks, margin, gap, sgap, n_zero)
                if ok:
                    break
                attempt += 1
                redraws += 1
            for k, v in zip(("preds", "maxvals", "center", "scale", "area", "box_score"), (preds, maxvals, center, scale, area, box)):
                cols[k].append(v)
            for c in COMBOS:
                scores, kh, ks, margin, gap, sgap, n_zero = res[c]
                d = per[c]
                d["score"].append(scores)
                d["keep_hard"].append(kh)
                d["keep_soft"].append(ks)
                d["margin"], d["gap"], d["score_gap"] = min(d["margin"], margin), min(d["gap"], gap), min(d["score_gap"], sgap)
                d["zero_max"] = max(d["zero_max"], n_zero)
            print("J=%d P=%d ok after %d redraw(s)" % (J, P, attempt), flush=True)
        pre = "j%d_" % J
        for k, v in cols.items():
            data[pre + k] = np.concatenate(v, 0)
        data[pre + "sigmas"] = sig[J]
        data[pre + "redraws"] = np.int32(redraws)
        for (thr, vis), d in per.items():
            q = "%st%g_v%g_" % (pre, thr, vis)
            data[q + "score"] = np.concatenate(d["score"])
            for name in ("keep_hard", "keep_soft"):
                data[q + name] = np.asarray([k for ks in d[name] for k in ks], np.int16)
                data[q + name + "_n"] = np.asarray([len(ks) for ks in d[name]], np.int16)
            data[q + "min_oks_margin"], data[q + "min_soft_gap"] = np.float64(d["margin"]), np.float64(d["gap"])
            data[q + "min_score_gap"], data[q + "max_invisible_persons"] = np.float64(d["score_gap"]), np.int32(d["zero_max"])
            n_sup = sum(P - len(k) for P, k in zip(COUNTS, d["keep_hard"]))
            n_kept = sum(len(k) for k in d["keep_hard"])
            assert n_sup > 0 and n_kept > 0, (J, thr, vis)  # (e)
            print("J=%d thr=%g vis=%g: kept %d, suppressed %d, min margin %.3g, min soft gap %.3g" % (J, thr, vis, n_kept, n_sup, d["margin"], d["gap"]))
    path = os.path.join(ROOT, "tests", "golden", "nms_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
