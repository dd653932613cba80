"""numpy restatement of i2r_val_combine: the loss / PCK accuracy of a whole batch from the rows (n_crops, sse[J], hits[J], valid[J]) of
its parts, as include/i2r_hip.h states it -- totals added in ascending part index, then the tail of i2r_val_metrics.  Shares no code
with the package; tests/test_val_combine.py holds it against the reference's own output cut into shards."""
import numpy as np


class Result:
    pass


def row(n_crops, sse=None, hits=None, valid=None, J=None):
    """one part's contribution, float64 [1 + 3 J]; a part without crops: row(0, J=J) -> zeros"""
    if sse is None:
        return np.zeros(1 + 3 * J)
    return np.concatenate([[float(n_crops)], np.asarray(sse, np.float64), np.asarray(hits, np.float64), np.asarray(valid, np.float64)])


def combine(parts, h, w, meter=None):
    """parts float64 [n_part, 1 + 3 J] -> Result with n_crops, sse, hits, valid, loss, acc [J + 1], avg_acc, cnt.  meter: a list of four
    floats, updated in place as validate()'s two AverageMeters are (not when there is no crop)."""
    parts = np.asarray(parts, np.float64)
    J = (parts.shape[1] - 1) // 3
    assert parts.ndim == 2 and parts.shape[1] == 1 + 3 * J and J >= 1
    r = Result()
    crops = 0.0
    r.sse, hits, valid = np.zeros(J), np.zeros(J), np.zeros(J)
    for p in parts:                       # ascending part index, one addition per part and joint
        if not p[0] > 0:
            continue
        crops += p[0]
        for j in range(J):
            r.sse[j] += p[1 + j]
            hits[j] += p[1 + J + j]
            valid[j] += p[1 + 2 * J + j]
    r.n_crops, r.hits, r.valid = int(crops), hits.astype(np.int32), valid.astype(np.int32)
    r.acc = np.zeros(J + 1)
    r.loss, r.avg_acc, r.cnt = 0.0, 0.0, 0
    if r.n_crops == 0:
        return r
    n_px = float(r.n_crops) * float(h) * float(w)
    loss, avg, cnt = 0.0, 0.0, 0
    for j in range(J):
        loss += 0.5 * (float(r.sse[j]) / n_px)
        v = float(r.hits[j]) * 1.0 / float(r.valid[j]) if r.valid[j] > 0 else -1.0
        r.acc[j + 1] = v
        if v >= 0:
            avg += v
            cnt += 1
    r.loss = loss / float(J)
    r.avg_acc = avg / float(cnt) if cnt != 0 else 0.0
    r.cnt = cnt
    r.acc[0] = r.avg_acc
    if meter is not None:
        meter[0] += r.loss * float(r.n_crops)
        meter[1] += float(r.n_crops)
        meter[2] += r.avg_acc * float(cnt)
        meter[3] += float(cnt)
    return r
