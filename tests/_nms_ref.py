"""Restatement of the reference's rescoring and OKS-NMS in float64 numpy (lib/dataset/coco.py:384-396, lib/nms/nms.py:75-181), used for
inputs tests/golden/nms_reference.npz does not hold.  tests/test_nms.py pins it to that fixture, which the reference's own functions
wrote (tools/make_golden_nms.py): every `keep` list equal, every score, cast to float32, equal.

Equal scores: the reference sorts with argsort()[::-1] of an unstable sort, so its order is undefined there; here (and in the kernel)
the person with the lower crop index comes first."""
import numpy as np

EPS = np.spacing(1)


def rescore(maxvals, box_score, in_vis_thre):
    """maxvals [P, J] float32, box_score [P] -> float64 [P]: (float32 mean of the joints above in_vis_thre, added in ascending order)
    * box_score.  The product of two float32 values is exact in float64, so its float32 cast is the correctly rounded fp32 product."""
    mv = np.asarray(maxvals, np.float32)
    mv = mv.reshape(mv.shape[0], -1) if mv.size else mv.reshape(0, 0)
    out = np.zeros(len(box_score), np.float64)
    for p in range(mv.shape[0]):
        s, n = np.float32(0), 0
        for j in range(mv.shape[1]):
            if float(mv[p, j]) > in_vis_thre:
                s = np.float32(s + mv[p, j])
                n += 1
        if n:
            s = np.float32(s / np.float32(n))
        out[p] = float(s) * float(box_score[p])
    return out


def oks_iou(g, d, a_g, a_d, sigmas, in_vis_thre=None):
    """g [J, 3], d [n, J, 3] (x, y, v) -> float64 [n].  dx, dy and dx^2 + dy^2 in float32 (the reference's key points are float32
    arrays), the rest in float64.  The joint mask is the candidate's alone: nms.py:95 `list(vg > t) and list(vd > t)` is its second operand."""
    g = np.asarray(g, np.float32)
    d = np.asarray(d, np.float32)
    var = (np.asarray(sigmas, np.float64) * 2) ** 2
    out = np.zeros(d.shape[0])
    for n in range(d.shape[0]):
        dx = d[n, :, 0] - g[:, 0]
        dy = d[n, :, 1] - g[:, 1]
        e = (dx * dx + dy * dy).astype(np.float64) / var / ((float(a_g) + float(a_d[n])) / 2 + EPS) / 2
        if in_vis_thre is not None:
            e = e[d[n, :, 2] > np.float32(in_vis_thre)]
        out[n] = np.sum(np.exp(-e)) / e.shape[0] if e.shape[0] else 0.0
    return out


def _order(scores):
    """descending score, equal scores by ascending index"""
    return np.lexsort((np.arange(len(scores)), -np.asarray(scores, np.float64)))


def oks_nms(kpts, scores, areas, thresh, sigmas, in_vis_thre=None, margins=None):
    """kpts [P, J, 3] -> keep list (nms.py:101-128).  margins: a list that receives |oks - thresh| of every comparison."""
    kpts = np.asarray(kpts, np.float32)
    areas = np.asarray(areas, np.float64)
    order = _order(scores)
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        ov = oks_iou(kpts[i], kpts[order[1:]], areas[i], areas[order[1:]], sigmas, in_vis_thre)
        if margins is not None:
            margins.extend(np.abs(ov - thresh).tolist())
        order = order[np.where(ov <= thresh)[0] + 1]
    return keep


def soft_oks_nms(kpts, scores, areas, thresh, sigmas, in_vis_thre=None, max_dets=20, gaps=None):
    """-> keep list (nms.py:142-181, Gaussian rescoring).  gaps: a list that receives (top - runner-up) / top of the decayed scores at
    every step that has a runner-up."""
    kpts = np.asarray(kpts, np.float32)
    areas = np.asarray(areas, np.float64)
    order = _order(scores)
    sc = np.asarray(scores, np.float64)[order]
    keep = []
    while order.size > 0 and len(keep) < max_dets:
        if gaps is not None and order.size > 1:
            gaps.append((sc[0] - sc[1]) / sc[0] if sc[0] > 0 else 0.0)
        i = order[0]
        ov = oks_iou(kpts[i], kpts[order[1:]], areas[i], areas[order[1:]], sigmas, in_vis_thre)
        order = order[1:]
        sc = sc[1:] * np.exp(-ov ** 2 / thresh)
        t = np.lexsort((order, -sc))
        order, sc = order[t], sc[t]
        keep.append(int(i))
    return keep


def run_batch(preds, maxvals, area, box_score, length, sigmas, in_vis_thre, oks_thre, soft=False, oks_vis_thre=None, max_dets=20):
    """The kernel's outputs for a batch: (score float32 [S], rank int32 [S], n_keep int32 [n_img])."""
    preds = np.asarray(preds, np.float32)
    S, J = preds.shape[0], preds.shape[1]
    mv = np.asarray(maxvals, np.float32).reshape(S, J)
    kp = np.concatenate([preds, mv[:, :, None]], 2)
    score = np.zeros(S, np.float32)
    rank = np.full(S, -1, np.int32)
    n_keep = np.zeros(len(length), np.int32)
    o = 0
    for i, n in enumerate(length):
        sc = rescore(mv[o:o + n], np.asarray(box_score)[o:o + n], in_vis_thre)
        score[o:o + n] = sc.astype(np.float32)
        if soft:
            keep = soft_oks_nms(kp[o:o + n], sc, np.asarray(area)[o:o + n], oks_thre, sigmas, oks_vis_thre, max_dets)
        else:
            keep = oks_nms(kp[o:o + n], sc, np.asarray(area)[o:o + n], oks_thre, sigmas, oks_vis_thre)
        for k, p in enumerate(keep):
            rank[o + p] = k
        n_keep[i] = len(keep)
        o += n
    return score, rank, n_keep
