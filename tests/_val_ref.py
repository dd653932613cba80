"""numpy restatement of the reference's per-batch validation numbers, for inputs tests/golden/val_metrics_reference.npz does not hold:
generate_target + adjust_target_weight (lib/dataset/JointsDataset.py:394-450), JointsMSELoss.forward (lib/core/loss.py:15-41, fp32 terms
summed in float64) and accuracy / calc_dists / dist_acc / get_max_preds (lib/core/evaluate.py:16-71, lib/core/inference.py:20-48).
tests/test_val_metrics.py holds it against the reference's own output."""
import numpy as np


def joint_targets(joints_hm, joints_vis, h, w, sigma=2, joints_weight=None):
    """joints_hm float64 [S, J, 2], joints_vis [S, J] -> (target fp32 [S, J, h, w], target_weight fp32 [S, J])"""
    mu = np.asarray(joints_hm, np.float64)
    S, J = mu.shape[:2]
    tw = np.array(joints_vis, np.float32).reshape(S, J).copy()
    target = np.zeros((S, J, h, w), np.float32)
    tmp = sigma * 3
    x = np.arange(w, dtype=np.float64)
    y = np.arange(h, dtype=np.float64)[:, None]
    for s in range(S):
        for j in range(J):
            mx, my = mu[s, j]
            if int(mx - tmp) >= w or int(my - tmp) >= h or int(mx + tmp + 1) < 0 or int(my + tmp + 1) < 0:
                tw[s, j] = 0
            if tw[s, j] > 0.5:
                target[s, j] = np.exp(-((x - mx) ** 2 + (y - my) ** 2) / (2 * sigma ** 2))   # float64, rounded once
    if joints_weight is not None:
        tw = tw * np.asarray(joints_weight, np.float32).reshape(1, J)
    return target, tw.astype(np.float32)


def max_preds(maps):
    """get_max_preds: fp32 [S, J, 2] = (idx % w, floor(idx / w)) of the first maximum, zeroed where the maximum is not > 0"""
    S, J, h, w = maps.shape
    flat = maps.reshape(S, J, -1)
    idx = np.argmax(flat, 2)
    mx = np.take_along_axis(flat, idx[:, :, None], 2)[:, :, 0]
    preds = np.stack([idx % w, idx // w], 2).astype(np.float32)
    return preds * (mx > 0.0)[:, :, None].astype(np.float32)


def sse_terms(output, target, target_weight, use_target_weight=True):
    """the fp32 squared differences as torch rounds them, [S, J, h*w] float32"""
    S, J = output.shape[:2]
    p = np.asarray(output, np.float32).reshape(S, J, -1)
    t = np.asarray(target, np.float32).reshape(S, J, -1)
    if use_target_weight:
        wt = np.asarray(target_weight, np.float32).reshape(S, J, 1)
        d = p * wt - t * wt
    else:
        d = p - t
    assert d.dtype == np.float32
    return d * d


class Result:
    pass


def val_metrics(output, target, target_weight, use_target_weight=True, dists_out=None):
    """-> Result with sse [J], loss (float64 sums of the fp32 terms), hits, valid, acc [J + 1], avg_acc, cnt, pred [S, J, 2]"""
    S, J, h, w = output.shape
    r = Result()
    r.sse = sse_terms(output, target, target_weight, use_target_weight).astype(np.float64).sum((0, 2))
    loss = 0.0
    for j in range(J):
        loss += 0.5 * (r.sse[j] / (float(S) * h * w))
    r.loss = loss / J
    r.pred = max_preds(np.asarray(output, np.float32))
    tp = max_preds(np.asarray(target, np.float32))
    n = np.array([h, w], np.float64) / 10
    r.hits, r.valid, r.acc = np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(J + 1)
    avg, cnt = 0.0, 0
    for j in range(J):
        for s in range(S):
            if tp[s, j, 0] > 1 and tp[s, j, 1] > 1:
                d = r.pred[s, j].astype(np.float64) / n - tp[s, j].astype(np.float64) / n
                dist = np.sqrt(d[0] * d[0] + d[1] * d[1])
                if dists_out is not None:
                    dists_out.append(dist)
                r.valid[j] += 1
                r.hits[j] += int(dist < 0.5)
        r.acc[j + 1] = r.hits[j] * 1.0 / r.valid[j] if r.valid[j] > 0 else -1
        if r.acc[j + 1] >= 0:
            avg += r.acc[j + 1]
            cnt += 1
    r.avg_acc = avg / cnt if cnt != 0 else 0.0
    r.cnt = cnt
    if cnt != 0:
        r.acc[0] = r.avg_acc
    return r


def host_path(output_dev, target_host, target_weight_host, use_target_weight=True):
    """what the device kernels replace, shaped like the reference's loop body: the device-to-host copy of the heat maps, the target
    upload, and the numpy path above (tools/time_val_metrics.py times it)"""
    out = output_dev.cpu().numpy()
    target_host.to(output_dev.device)
    return val_metrics(out, target_host.numpy(), target_weight_host.numpy(), use_target_weight)
