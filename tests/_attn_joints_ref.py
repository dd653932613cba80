"""numpy restatement of what i2r_joint_tokens computes (include/i2r_hip.h), sharing no code with the package: the literal get_max_preds of
the reference (lib/core/inference.py:20-48) -- np.argmax (first index), np.amax, the pred_mask that zeroes the point of a map without a
positive value -- then x in_stride into the frame of the crop's network input, then the token of visualize.py:194-196,
(int(y / down_rate), int(x / down_rate)) clamped to the token map, shifted by the person's place in its group."""
import numpy as np


def max_preds(hm):
    """inference.py:29-48, line by line -> (preds [S, J, 2] float32 (x, y) in heat-map pixels, maxvals [S, J] float32)"""
    S, J, width = hm.shape[0], hm.shape[1], hm.shape[3]
    flat = hm.reshape((S, J, -1))
    idx = np.argmax(flat, 2).reshape((S, J, 1))
    maxvals = np.amax(flat, 2).reshape((S, J, 1))
    preds = np.tile(idx, (1, 1, 2)).astype(np.float32)
    preds[:, :, 0] = (preds[:, :, 0]) % width
    preds[:, :, 1] = np.floor((preds[:, :, 1]) / width)
    preds *= np.tile(np.greater(maxvals, 0.0), (1, 1, 2)).astype(np.float32)
    return preds, maxvals.reshape(S, J)


def crop_places(length, intra):
    """(group, slot) of every crop: an intra-human stack groups by crop, the inter-human stack by image (slot = person in the image)"""
    S = int(sum(length))
    if intra:
        return list(range(S)), [0] * S
    return [b for b, n in enumerate(length) for _ in range(n)], [p for n in length for p in range(n)]


def joint_tokens(hm, in_stride, tables):
    """hm [S, J, hh, hw] float32; tables: dicts(n_grp, K, fh, fw, down, group [S], slot [S]) -> (points [S, J, 2] float32 in input pixels,
    maxvals [S, J], per table the int32 [n_grp, K] tokens, -1 where no crop writes)"""
    preds, maxvals = max_preds(np.asarray(hm, dtype=np.float32))
    points = preds * np.float32(in_stride)
    S, J = maxvals.shape
    out = []
    for t in tables:
        tok = np.full((t["n_grp"], t["K"]), -1, dtype=np.int32)
        for s in range(S):
            g, slot = t["group"][s], t["slot"][s]
            for j in range(J):
                x, y = float(points[s, j, 0]), float(points[s, j, 1])
                row, col = min(int(y / t["down"]), t["fh"] - 1), min(int(x / t["down"]), t["fw"] - 1)
                tok[g, slot * J + j] = slot * t["fh"] * t["fw"] + row * t["fw"] + col
        out.append(tok)
    return points, maxvals, out


def edge_maps(S, J, hh, hw, seed):
    """seeded maps [S, J, hh, hw] float32 holding, by turns over the S * J maps: a two-pixel tie of the maximum (the first must win), the
    maximum at the last pixel, an all-negative map, an all-zero map, and plain seeded maps with a positive peak"""
    rng = np.random.RandomState(seed)
    hm = rng.uniform(-1.0, 0.5, size=(S, J, hh, hw)).astype(np.float32)
    flat = hm.reshape(S * J, hh * hw)
    n = hh * hw
    for i in range(S * J):
        kind = i % 5
        if kind == 0 and n >= 2:
            a, b = sorted(rng.choice(n, size=2, replace=False))
            flat[i, a] = flat[i, b] = np.float32(0.75)
        elif kind == 1:
            flat[i, n - 1] = np.float32(0.875)
        elif kind == 2:
            flat[i] = -np.abs(flat[i]) - np.float32(0.125)
        elif kind == 3:
            flat[i] = 0.0
        else:
            flat[i, rng.randint(n)] = np.float32(0.625)
    return hm
