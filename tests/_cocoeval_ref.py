"""A literal numpy float64 restatement of the key-point path of the published pycocotools (coco.py loadRes, cocoeval.py _prepare,
computeOks, evaluateImg, accumulate, summarize / _summarizeKps), for one category, with its data structures (lists of dicts, per-image
Python loops).  Written for reading, not speed; it shares no code with i2r_amd.caller.  pycocotools itself is not available to this
project, so this file is the yardstick of the device evaluation and is held in place by the hand-derived cases of tests/test_oks_eval.py.

    gts: list of dicts  image_id, keypoints [x, y, v] * J, area, bbox [x, y, w, h], iscrowd, num_keypoints   (the annotation file)
    dts: list of dicts  image_id, keypoints [x, y, v] * J, score                                                (the result file)"""
import copy

import numpy as np

KPT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0
STATS_NAMES = ["AP", "Ap .5", "AP .75", "AP (M)", "AP (L)", "AR", "AR .5", "AR .75", "AR (M)", "AR (L)"]


class Params:
    """Params.setKpParams"""

    def __init__(self, sigmas=None):
        self.imgIds = []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [20]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ["all", "medium", "large"]
        self.kpt_oks_sigmas = KPT_OKS_SIGMAS if sigmas is None else np.asarray(sigmas, np.float64)


def load_res(dts, gt_image_ids):
    """COCO.loadRes, the 'keypoints' branch: area and bbox of a result from the extent of its points, ids from 1"""
    anns = copy.deepcopy(dts)
    assert set(a["image_id"] for a in anns) == (set(a["image_id"] for a in anns) & set(gt_image_ids)), \
        "Results do not correspond to current coco set"
    for id, ann in enumerate(anns):
        s = ann["keypoints"]
        x = s[0::3]
        y = s[1::3]
        x0, x1, y0, y1 = np.min(x), np.max(x), np.min(y), np.max(y)
        ann["area"] = (x1 - x0) * (y1 - y0)
        ann["id"] = id + 1
        ann["bbox"] = [x0, y0, x1 - x0, y1 - y0]
    return anns


class CocoEvalRef:
    def __init__(self, gts, dts, image_ids, sigmas=None):
        """image_ids: the ids of the annotation file's images (an image without annotations is still evaluated)"""
        self.params = Params(sigmas)
        self.params.imgIds = sorted(image_ids)
        self.gts_in = copy.deepcopy(gts)
        for i, g in enumerate(self.gts_in):
            g.setdefault("id", i + 1)
        self.dts_in = load_res(dts, image_ids)

    def _prepare(self):
        """COCOeval._prepare"""
        p = self.params
        ids = set(p.imgIds)
        gts = [g for g in self.gts_in if g["image_id"] in ids]
        dts = [d for d in self.dts_in if d["image_id"] in ids]
        for gt in gts:
            gt["ignore"] = gt["ignore"] if "ignore" in gt else 0
            gt["ignore"] = "iscrowd" in gt and gt["iscrowd"]
            gt["ignore"] = (gt["num_keypoints"] == 0) or gt["ignore"]
        self._gts = {i: [] for i in p.imgIds}
        self._dts = {i: [] for i in p.imgIds}
        for gt in gts:
            self._gts[gt["image_id"]].append(gt)
        for dt in dts:
            self._dts[dt["image_id"]].append(dt)
        self.evalImgs = []
        self.eval = {}

    def evaluate(self):
        """COCOeval.evaluate"""
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        self.ious = {imgId: self.computeOks(imgId) for imgId in p.imgIds}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(imgId, areaRng, maxDet) for areaRng in p.areaRng for imgId in p.imgIds]

    def computeOks(self, imgId):
        """COCOeval.computeOks"""
        p = self.params
        gts = self._gts[imgId]
        dts = self._dts[imgId]
        inds = np.argsort([-d["score"] for d in dts], kind="mergesort")
        dts = [dts[i] for i in inds]
        if len(dts) > p.maxDets[-1]:
            dts = dts[0:p.maxDets[-1]]
        if len(gts) == 0 or len(dts) == 0:
            return []
        ious = np.zeros((len(dts), len(gts)))
        sigmas = p.kpt_oks_sigmas
        vars = (sigmas * 2) ** 2
        k = len(sigmas)
        for j, gt in enumerate(gts):
            g = np.array(gt["keypoints"])
            xg = g[0::3]
            yg = g[1::3]
            vg = g[2::3]
            k1 = np.count_nonzero(vg > 0)
            bb = gt["bbox"]
            x0 = bb[0] - bb[2]
            x1 = bb[0] + bb[2] * 2
            y0 = bb[1] - bb[3]
            y1 = bb[1] + bb[3] * 2
            for i, dt in enumerate(dts):
                d = np.array(dt["keypoints"])
                xd = d[0::3]
                yd = d[1::3]
                if k1 > 0:
                    dx = xd - xg
                    dy = yd - yg
                else:
                    z = np.zeros((k))
                    dx = np.max((z, x0 - xd), axis=0) + np.max((z, xd - x1), axis=0)
                    dy = np.max((z, y0 - yd), axis=0) + np.max((z, yd - y1), axis=0)
                e = (dx ** 2 + dy ** 2) / vars / (gt["area"] + np.spacing(1)) / 2
                if k1 > 0:
                    e = e[vg > 0]
                ious[i, j] = np.sum(np.exp(-e)) / e.shape[0]
        return ious

    def evaluateImg(self, imgId, aRng, maxDet):
        """COCOeval.evaluateImg"""
        p = self.params
        gt = self._gts[imgId]
        dt = self._dts[imgId]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            if g["ignore"] or (g["area"] < aRng[0] or g["area"] > aRng[1]):
                g["_ignore"] = 1
            else:
                g["_ignore"] = 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:maxDet]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        ious = self.ious[imgId][:, gtind] if len(self.ious[imgId]) > 0 else self.ious[imgId]
        T = len(p.iouThrs)
        G = len(gt)
        D = len(dt)
        gtm = np.zeros((T, G))
        dtm = np.zeros((T, D))
        gtIg = np.array([g["_ignore"] for g in gt])
        dtIg = np.zeros((T, D))
        if not len(ious) == 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind, g in enumerate(gt):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = d["id"]
        a = np.array([d["area"] < aRng[0] or d["area"] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"image_id": imgId, "aRng": aRng, "maxDet": maxDet, "dtIds": [d["id"] for d in dt], "gtIds": [g["id"] for g in gt],
                "dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gtIg, "dtIgnore": dtIg}

    def accumulate(self):
        """COCOeval.accumulate (one category)"""
        p = self.params
        T = len(p.iouThrs)
        R = len(p.recThrs)
        A = len(p.areaRng)
        M = len(p.maxDets)
        precision = -np.ones((T, R, 1, A, M))
        recall = -np.ones((T, 1, A, M))
        npigs = np.zeros((A,), np.int64)
        I0 = len(p.imgIds)
        for a in range(A):
            Na = a * I0
            for m, maxDet in enumerate(p.maxDets):
                E = [self.evalImgs[Na + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dtScores = np.concatenate([e["dtScores"][0:maxDet] for e in E])
                inds = np.argsort(-dtScores, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                dtIg = np.concatenate([e["dtIgnore"][:, 0:maxDet] for e in E], axis=1)[:, inds]
                gtIg = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtIg == 0)
                npigs[a] = npig
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtIg))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                precision[:, :, 0, a, m], recall[:, 0, a, m] = accumulate_flags(tps, fps, npig, p.recThrs)
        self.eval = {"precision": precision, "recall": recall, "npig": npigs}

    def summarize(self):
        """COCOeval.summarize -> _summarizeKps"""
        p = self.params

        def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
            aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
            mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
            if ap == 1:
                s = self.eval["precision"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, :, aind, mind]
            else:
                s = self.eval["recall"]
                if iouThr is not None:
                    t = np.where(iouThr == p.iouThrs)[0]
                    s = s[t]
                s = s[:, :, aind, mind]
            if len(s[s > -1]) == 0:
                mean_s = -1
            else:
                mean_s = np.mean(s[s > -1])
            return mean_s
        stats = np.zeros((10,))
        stats[0] = _summarize(1, maxDets=20)
        stats[1] = _summarize(1, maxDets=20, iouThr=.5)
        stats[2] = _summarize(1, maxDets=20, iouThr=.75)
        stats[3] = _summarize(1, maxDets=20, areaRng="medium")
        stats[4] = _summarize(1, maxDets=20, areaRng="large")
        stats[5] = _summarize(0, maxDets=20)
        stats[6] = _summarize(0, maxDets=20, iouThr=.5)
        stats[7] = _summarize(0, maxDets=20, iouThr=.75)
        stats[8] = _summarize(0, maxDets=20, areaRng="medium")
        stats[9] = _summarize(0, maxDets=20, areaRng="large")
        self.stats = stats
        return stats


def accumulate_flags(tps, fps, npig, recThrs):
    """the inner part of COCOeval.accumulate from `tp_sum = np.cumsum(...)` on: tps, fps bool [T, nd] in sorted order
    -> precision [T, R], recall [T]"""
    T = tps.shape[0]
    R = len(recThrs)
    precision = np.zeros((T, R))
    recall = np.zeros((T,))
    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
        tp = np.array(tp)
        fp = np.array(fp)
        nd = len(tp)
        rc = tp / npig
        pr = tp / (fp + tp + np.spacing(1))
        q = np.zeros((R,))
        if nd:
            recall[t] = rc[-1]
        else:
            recall[t] = 0
        pr = pr.tolist()
        q = q.tolist()
        for i in range(nd - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        inds = np.searchsorted(rc, recThrs, side="left")
        try:
            for ri, pi in enumerate(inds):
                q[ri] = pr[pi]
        except Exception:
            pass
        precision[t, :] = np.array(q)
    return precision, recall


def run(gts, dts, image_ids, sigmas=None):
    """evaluate + accumulate + summarize -> the CocoEvalRef (stats, eval, evalImgs, ious)"""
    e = CocoEvalRef(gts, dts, image_ids, sigmas)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


def run_subset(gts, dts, image_ids, keep_ids, sigmas=None):
    """what KeypointEvaluator does with files: annotation and result files cut down to the images of one level, then the same evaluation"""
    keep = set(keep_ids)
    return run([g for g in gts if g["image_id"] in keep], [d for d in dts if d["image_id"] in keep], [i for i in image_ids if i in keep], sigmas)
