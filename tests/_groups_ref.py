"""numpy restatement of the grouped test modes of the reference's collater (lib/dataset/collater.py:28-95,164-173), the yardstick of
i2r_group_nearest and input.window_lengths.  tests/test_groups.py holds it equal to the reference's own output
(tests/golden/groups_reference.json, written by tools/make_golden_groups.py from the imported reference).

main_target: per image of n persons with anchors a_i = (box_i[0], box_i[1]) and p = max_patch
    n == 1: one group [0]; else per target t a group of k = min(n, p): t, then the k - 1 persons j != t smallest by (d(t, j), j),
    d = (ax_t - ax_j)^2 + (ay_t - ay_j)^2 in float64, every operation rounded on its own (numpy does exactly that).
The reference sorts ALL persons, the target included, by np.linalg.norm (stable): the same order unless another person shares the
target's anchor -- then it may put that person first, or leave the target out; the definition here keeps the target first, always."""
import numpy as np


def main_target(anchors, length, max_patch):
    """anchors: float64 [S, 2]; length: persons per image -> (groups: list of lists of GLOBAL person indices, one per person of the
    batch, target first; group_len)"""
    p = int(max_patch)
    if p < 1:
        raise ValueError("max_patch must be >= 1")
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 2)
    groups, s = [], 0
    for n in length:
        n = int(n)
        if n == 1:
            groups.append([s])
        else:
            k = min(n, p)
            ax, ay = a[s:s + n, 0], a[s:s + n, 1]
            for t in range(n):
                dx, dy = ax[t] - ax, ay[t] - ay
                d = dx * dx + dy * dy  # (three separate roundings per element)
                others = sorted((j for j in range(n) if j != t), key=lambda j: (d[j], j))
                groups.append([s + t] + [s + j for j in others[:k - 1]])
        s += n
    assert s == a.shape[0]
    return groups, [len(g) for g in groups]


def window(length, max_patch):
    """-> the `length` list of the window mode: images of more than max_patch persons cut into consecutive chunks of max_patch (the
    crops keep their order)"""
    p = int(max_patch)
    if p < 1:
        raise ValueError("max_patch must be >= 1")
    out = []
    for n in length:
        n = int(n)
        out += [min(p, n - i) for i in range(0, n, p)] if n > p else [n]
    return out


def layout(length, max_patch):
    """(group_len, person_off, member_off) from the person counts alone"""
    p = int(max_patch)
    group_len, person_off, member_off = [], [0], [0]
    for n in length:
        k = 1 if n == 1 else min(n, p)
        group_len += [k] * n
        person_off.append(person_off[-1] + n)
        member_off.append(member_off[-1] + n * k)
    return group_len, person_off, member_off


def mixed_anchors(length, seed=0, ties=True):
    """distinct anchors on a quarter-pixel grid below 4096 for images of `length` persons (every d exact in float64), with planted
    equal-distance pairs: in every image of >= 3 persons, persons 1 and 2 lie 5 px from person 0 ((3, 4) and (5, 0)), and in larger
    images a few HIGH-index persons mirror LOW-index ones about a third person."""
    rng = np.random.RandomState(seed)
    out = []
    for n in length:
        while True:
            a = rng.randint(64, 4096 * 4 - 64, size=(n, 2)).astype(np.float64) / 4.0
            if ties and n >= 3:
                a[1] = a[0] + (3.0, 4.0)
                a[2] = a[0] + (5.0, 0.0)
            if ties and n >= 8:
                for c, lo, hi in ((3, 4, n - 1), (5, 6, n - 2)):
                    a[hi] = 2.0 * a[c] - a[lo]  # (mirror of person lo about person c: equally far from c)
            if len({tuple(r) for r in a}) == n and a.min() >= 0 and a.max() < 4096:
                break
        out.append(a)
    return np.concatenate(out) if out else np.zeros((0, 2))
