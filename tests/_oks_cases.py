"""Cases shared by tests/test_oks_eval.py and tests/test_oks_eval_gpu.py: the hand-derived cases whose numbers stand here as fractions, the
lists-of-dicts -> annotation-file helper, the seeded generator of the GPU tests and the margin recorder that decides whether a drawn
image is kept.  The recorder replays evaluateImg's walk on the restatement's own OKS matrices; tests/_cocoeval_ref.py itself carries
no instrumentation."""
from fractions import Fraction

import numpy as np

import _cocoeval_ref as ref

SIGMAS14 = tuple(v / 10.0 for v in (.79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89, .62, .79))[::-1]   # a second table, J = 14
MARGIN = 1e-9


# ---- hand-derived cases -------------------------------------------------------------------------------------------------------------
def pose(cx, cy, J=17, v=2):
    """J points on a 10 px lattice, 5 per row, from (cx, cy): extent 40 x 30 for J = 17 (a detection area of 1200: 'medium')"""
    return [c for j in range(J) for c in (float(cx + 10 * (j % 5)), float(cy + 10 * (j // 5)), v)]


def gt_of(img, cx, cy, area=2500.0, iscrowd=0, v=2, bbox=None):
    kp = pose(cx, cy, v=v)
    return dict(image_id=img, keypoints=kp, area=float(area), bbox=bbox or [float(cx), float(cy), 40.0, 30.0], iscrowd=iscrowd,
                num_keypoints=sum(1 for x in kp[2::3] if x > 0))


def dt_of(img, cx, cy, score):
    return dict(image_id=img, keypoints=pose(cx, cy, v=1), score=score)


FAR = 5000   # px between unrelated poses: OKS exactly 0


def hand_cases():
    """name -> (gts, dts, image ids, the ten stats as Fractions).  Every gt has area 2500 (medium) unless the case is about areas."""
    c = {}
    one, none, half, zero = Fraction(1), Fraction(-1), Fraction(1, 2), Fraction(0)
    medium = lambda ap, ar: [ap, ap, ap, ap, none, ar, ar, ar, ar, none]
    # one gt, one exact detection: everything of its area class is 1, the class it is not in stays -1
    c["exact"] = ([gt_of(7, 100, 100)], [dt_of(7, 100, 100, 0.9)], [7], medium(one, one))
    # two gts; TP(.9) FP(.8) TP(.7): rc = 1/2, 1/2, 1; pr = 1, 1/2, 2/3 -> 1, 2/3, 2/3: 51 recall thresholds (0 ... 0.5) see 1, 50 see 2/3
    ap = (51 + 50 * Fraction(2, 3)) / 101
    c["tp_fp_tp"] = ([gt_of(1, 100, 100), gt_of(1, 100 + FAR, 100)],
                     [dt_of(1, 100, 100, 0.9), dt_of(1, 100, 100 + FAR, 0.8), dt_of(1, 100 + FAR, 100, 0.7)], [1], medium(ap, one))
    # a detection (the best scored one) on an image without gt: pr = 0, 1/2 -> 1/2, 1/2; the recall is not touched
    c["image_without_gt"] = ([gt_of(1, 100, 100)], [dt_of(1, 100, 100, 0.9), dt_of(2, 100, 100, 0.95)], [1, 2], medium(half, one))
    # a crowd gt absorbs the two best scored detections: both ignored (as false positives they would halve the precision of the third)
    c["crowd"] = ([gt_of(1, 100, 100), gt_of(1, 100 + FAR, 100, iscrowd=1)],
                  [dt_of(1, 100 + FAR, 100, 0.95), dt_of(1, 100 + FAR, 100, 0.92), dt_of(1, 100, 100, 0.9)], [1], medium(one, one))
    # a gt without labelled points is ignored and scored through its bbox (x - w ... x + 2 w): the detection inside that box matches it
    # (OKS 1) and is ignored; the one outside is a false positive in front of the true positive: pr = 0, 1/2 (1/3 were the first one counted)
    c["no_keypoints"] = ([gt_of(1, 100, 100), gt_of(1, 100 + FAR, 100, v=0, bbox=[100.0 + FAR, 100.0, 40.0, 30.0])],
                         [dt_of(1, 100 + FAR - 30, 100 + 20, 0.95), dt_of(1, 100 + 3 * FAR, 100, 0.93), dt_of(1, 100, 100, 0.9)], [1],
                         medium(half, one))
    # area exactly 96^2: inside 'medium' [32^2, 96^2] and inside 'large' [96^2, 1e10], bounds inclusive
    c["area_on_the_bound"] = ([gt_of(1, 100, 100, area=96.0 ** 2)], [dt_of(1, 100, 100, 0.9)], [1], [one] * 10)
    # 21 detections: the 20 best scored ones are false positives, the true positive is the 21st and is cut (1/21 were it seen)
    c["cut_at_20"] = ([gt_of(1, 100, 100)], [dt_of(1, 100, 100, 0.1)] + [dt_of(1, 100 + FAR * (i + 1), 100, 0.9 - i / 64) for i in range(20)],
                      [1], medium(zero, zero))
    # equal scores keep the input order (a stable sort): FP in front of TP -> pr = 0, 1/2; TP in front of FP -> 1
    c["tie_fp_first"] = ([gt_of(1, 100, 100)], [dt_of(1, 100 + FAR, 100, 0.75), dt_of(1, 100, 100, 0.75)], [1], medium(half, one))
    c["tie_tp_first"] = ([gt_of(1, 100, 100)], [dt_of(1, 100, 100, 0.75), dt_of(1, 100 + FAR, 100, 0.75)], [1], medium(one, one))
    return c


HAND = hand_cases()


def coco_dict(gts, image_ids):
    anns = [dict(g, id=i + 1, category_id=1) for i, g in enumerate(gts)]
    return dict(images=[dict(id=i) for i in image_ids], annotations=anns, categories=[dict(id=1, name="person")])


def walk_margins(e):
    """Replays the greedy walk of evaluateImg on the finished evaluation `e` (its OKS matrices, ignore flags and orders) and returns
    (a) |oks - value it is compared with| of every comparison the walk makes (a threshold or the running iou) and (b) the gaps between
    those OKS values of one detection's row that can be accepted at all, i.e. lie at or above the lowest threshold - 1e-9: lower values
    never compete with anything, and the OKS of far-apart poses underflow to the same 0.  The replay must reproduce e's matches."""
    p = e.params
    out = []
    I = len(p.imgIds)
    for a in range(len(p.areaRng)):
        for i, imgId in enumerate(p.imgIds):
            E = e.evalImgs[a * I + i]
            if E is None or len(e.ious[imgId]) == 0:
                continue
            gt_ids = [g["id"] for g in e._gts[imgId]]
            cols = [gt_ids.index(g) for g in E["gtIds"]]
            crowd = {g["id"]: int(g["iscrowd"]) for g in e._gts[imgId]}
            iscrowd = [crowd[g] for g in E["gtIds"]]
            ious = e.ious[imgId][:, cols]
            gtIg = E["gtIgnore"]
            if a == 0:
                for row in ious:
                    s = np.sort(row[row >= p.iouThrs.min() - 1e-9])
                    out.extend(np.diff(s).tolist())
            for tind, t in enumerate(p.iouThrs):
                taken = np.zeros(len(cols), bool)
                for dind in range(ious.shape[0]):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(len(cols)):
                        if taken[gind] and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        out.append(abs(ious[dind, gind] - iou))
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    assert (m > -1) == (E["dtMatches"][tind, dind] != 0), "the replay follows evaluateImg"
                    if m > -1:
                        assert E["dtMatches"][tind, dind] == E["gtIds"][m]
                        taken[m] = True
    return out


# ---- the seeded generator of the GPU tests -------------------------------------------------------------------------------------------
def _grid(a):
    return np.round(np.asarray(a, np.float64) * 256.0) / 256.0   # key points on a 1/256 px grid: exact in fp32 up to 65536 px


AREAS_ON_PURPOSE = (32.0 ** 2, 96.0 ** 2, 32.0 ** 2 - 0.5, 96.0 ** 2 + 0.5, 500.0)   # on the bounds, just outside 'medium', below it


def draw_image(rng, img, n_dt, n_gt, J, sigmas, special=True, distinct_scores=False):
    """One image: n_gt persons on a 1200 px canvas (sizes 30 ... 250 px; crowd gts, gts without labelled points, areas in, between
    and exactly on the bounds of the ranges), n_dt detections = a gt plus jitter of 0.05 ... 100 px, or strays; scores on a 1/1024 grid,
    with ties.  Redrawn until the restatement's own comparisons (oks against a threshold or the running iou, and accepted values of
    one row against each other) all lie >= MARGIN apart.  -> (gts, dts, the achieved minimum)"""
    while True:
        gts, dts = [], []
        for _ in range(n_gt):
            size = rng.uniform(30, 250)
            kp = np.zeros((J, 3))
            kp[:, :2] = _grid(rng.uniform(0, 1200, 2) + rng.uniform(0, 1, (J, 2)) * size)
            kp[:, 2] = rng.choice([0, 1, 2], J, p=[.2, .3, .5])
            kind = rng.integers(0, 10) if special else 9
            if kind == 0:
                kp[:, 2] = 0                                        # no labelled point: ignored, scored through the bbox
            lo, hi = kp[:, :2].min(0), kp[:, :2].max(0)
            area = float(rng.choice(AREAS_ON_PURPOSE)) if kind == 1 else float(_grid((hi - lo).prod() * rng.uniform(.3, .8)))
            gts.append(dict(image_id=img, keypoints=kp.reshape(-1).tolist(), area=area, bbox=[lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]],
                            iscrowd=int(kind == 2), num_keypoints=int((kp[:, 2] > 0).sum())))
        for i in range(n_dt):
            if n_gt and rng.uniform() < .8:
                g = np.asarray(gts[rng.integers(0, n_gt)]["keypoints"]).reshape(J, 3)[:, :2]
                xy = g + rng.standard_normal((J, 2)) * 10.0 ** rng.uniform(np.log10(.05), 2)
            else:
                xy = rng.uniform(0, 1200, 2) + rng.uniform(0, 1, (J, 2)) * rng.uniform(20, 300)
            kp = np.concatenate([_grid(xy), np.ones((J, 1))], 1)
            dts.append(dict(image_id=img, keypoints=kp.reshape(-1).tolist(), score=float(rng.integers(1, 1024)) / 1024.0))
        if distinct_scores:
            for i, s in enumerate(rng.permutation(len(dts))):
                dts[i]["score"] = float(s + 1) / 2048.0 + img / 2.0 ** 20   # distinct inside the image and, with img < 512, across images
        elif special and n_dt > 2:
            dts[-1]["score"] = dts[0]["score"]                      # a tie on an exactly representable value
        margins = walk_margins(ref.run(gts, dts, [img], sigmas))
        low = min(margins) if margins else 1.0
        if low >= MARGIN:
            return gts, dts, low
