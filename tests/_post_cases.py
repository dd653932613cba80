"""Heat maps for the keypoint decode (csrc/i2r_post.hip: i2r_decode) at the places where such a kernel goes wrong, and their expected
values from oracle/post_cpu.py.  Used on the CPU (tests/test_post_oracle.py: the table must be able to tell the oracle from a set of
subtly wrong oracles, and every refined map must be well conditioned) and on the GPU (tests/test_post_gpu.py).

A case is a batch of maps [S, J, h, w] fp32, a blur size, and the crops' centres and scales [S, 2].  Families:
  skewed      rotated anisotropic Gaussians (the cross term dxy of the Taylor step is as large as dxx, dyy) alternating with two-lobe
              sums of a narrow and a wide Gaussian 1-2 px apart (not a quadratic in the log: the blur coefficients move the answer),
              and, at blur sizes 3, 5, 7, pixel combs (COMBS) on which the blur coefficients move the answer by a tenth of a pixel and more
  guards      a single dominant pixel + one inward diagonal neighbour on a smooth slope, the peak on every column / row next to the
              refinement guard 1 < px < w-2, 1 < py < h-2, and in the corners
  ties        two or three exactly equal maxima, placed against the 256-thread stride loop, the 64-lane butterfly and the four waves
  degenerate  maps without a usable peak; the decode must stay finite and on the integer position
  shapes      skewed peaks on maps below one workgroup's 256 threads, on odd sizes, and on the two sizes that need the dynamic-LDS opt-in
Everything is a pure function of synth.uniform01."""
import functools
import types

import numpy as np

import post_cpu
from i2r_amd import synth

TOL = 5e-3       # heat-map pixels, fp32 kernel against the float64 oracle (tests/test_post_gpu.py::test_decode_matches_oracle)
COND_MIN = 1e-3  # smallest |det| / (|dxx dyy| + dxy^2) a refined map of the table may have


def _u(key, n, seed=11):
    return synth.uniform01(seed, "post-cases/" + key, n)


def _gauss(h, w, cx, cy, s1, s2, theta):
    """exp(-q/2) of a Gaussian with standard deviations s1 (along theta) and s2 (across), float64 [h, w]"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    a = (xx - cx) * c + (yy - cy) * s
    b = -(xx - cx) * s + (yy - cy) * c
    return np.exp(-0.5 * ((a / s1) ** 2 + (b / s2) ** 2))


def skewed_maps(n, h, w, key, margin=None):
    """n maps: even ones a rotated anisotropic Gaussian (axis ratio 2..3, angles spread over 0..180 degrees), odd ones a two-lobe sum"""
    if margin is None:
        margin = 4 if min(h, w) >= 15 else 2
    u = _u(key, n * 8).reshape(n, 8)
    out = np.zeros((n, h, w), np.float32)
    for m in range(n):
        cx = margin + u[m, 0] * (w - 1 - 2 * margin)
        cy = margin + u[m, 1] * (h - 1 - 2 * margin)
        amp = 0.3 + 0.7 * u[m, 2]
        if m % 2 == 0:
            s2 = 1.0 + 0.6 * u[m, 3]
            s1 = s2 * (2.0 + u[m, 4])
            theta = np.pi * ((m // 2 + u[m, 5]) / max(1, (n + 1) // 2))
            g = amp * _gauss(h, w, cx, cy, s1, s2, theta)
        else:
            sa = 0.7 + 0.3 * u[m, 3]
            sb = 2.0 + u[m, 4]
            d, phi = 1.0 + u[m, 5], 2 * np.pi * u[m, 6]
            g = amp * (_gauss(h, w, cx, cy, sa, sa, 0.0)
                       + (0.6 + 0.3 * u[m, 7]) * _gauss(h, w, cx + d * np.cos(phi), cy + d * np.sin(phi), sb, sb, 0.0))
        out[m] = g
    return out


# rows of pixels around a peak of 1.0 (the middle entry) over a flat background (the last number): patterns whose sub-pixel answer depends on
# the blur coefficients themselves -- the first moves by 0.1 px between OpenCV's fixed 3-tap table and the Gaussian formula, the second
# and third do the same for 5 and 7 taps.  Each is laid along x and along y, in the cases of its own blur size.
COMBS = (((0.0, 0.95, 0.0, 1.0, 0.2, 0.8, 0.0), 1e-3),
         ((0.95, 0.95, 0.0, 1.0, 0.5, 0.5, 0.5), 0.1),
         ((0.95, 0.95, 0.0, 1.0, 0.5, 0.95, 0.5), 0.1))


COMB_OF_BLUR = {3: 0, 5: 1, 7: 2}


def comb_maps(h, w, ksize):
    """the comb of blur size `ksize`, along x and along y"""
    m = COMB_OF_BLUR[ksize]
    row, bg = COMBS[m]
    row = np.maximum(np.asarray(row, np.float32), np.float32(bg))
    y, x = h // 2 + m - 1, w // 2 - 3 + (m % 2)
    out = np.full((2, h, w), bg, np.float32)
    out[0, y, x:x + 7] = row
    out[1, y - 3:y + 4, x + 3] = row[::-1]
    return out


def guard_positions(h, w):
    """(px, py) of the peaks: every column next to the guard with an interior row, the transpose, the corners, and the two interior
    positions that touch the guard on both axes"""
    xs, ys = (0, 1, 2, w - 3, w - 2, w - 1), (0, 1, 2, h - 3, h - 2, h - 1)
    pos = [(x, h // 2) for x in xs] + [(w // 2, y) for y in ys]
    pos += [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (2, 2), (w - 3, h - 3)]
    return pos


def guard_maps(h, w):
    pos = guard_positions(h, w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((len(pos), h, w), np.float32)
    for m, (px, py) in enumerate(pos):
        g = 0.02 + 0.03 * (xx / (w - 1)) + 0.02 * (yy / (h - 1))      # smooth slope
        g[py, px] = 1.0
        sx, sy = (1 if px < w / 2 else -1), (1 if py < h / 2 else -1)  # the neighbour that points into the map
        g[py + sy, px + sx] = 0.6
        out[m] = g
    return out


# flat indices (i1 < i2 [< i3]) of equal maxima on a 64 x 48 map (3072 pixels: 12 per thread of the stride loop; thread = i % 256,
# wave = thread / 64)
TIES_64x48 = [
    (300, 513),          # threads 44 and 1: the later pixel sits in the lower thread, same wave
    (200, 260),          # threads 200 (wave 3) and 4 (wave 0): the later pixel in the lower wave
    (70, 70 + 256 * 5),  # the same thread's stride
    (10, 100),           # waves 0 and 1 in index order
    (1265, 1266),        # neighbouring lanes: a plateau of two pixels
    (2815, 3071),        # same thread (255), the last pixel of the map
    (700, 1500, 2900),   # three waves: 2, 3, 1
    (30 + 48 * 5, 30 + 48 * 5 + 256, 30 + 48 * 5 + 512),  # three in one thread
    (1000, 1000 + 64, 1000 + 128),                        # three waves of one pass of the stride loop, same lane
    (1500, 1535),        # threads 220 (wave 3) and 255 (wave 3): same wave, far lanes
]
TIES_96x72 = [(3000, 96 * 72 - 1), (96 * 72 - 2, 96 * 72 - 1)]


def tie_maps(h, w, ties):
    out = np.zeros((len(ties), h, w), np.float32)
    u = _u("ties%dx%d" % (h, w), len(ties) * 4).reshape(len(ties), 4)
    for m, idx in enumerate(ties):
        g = np.zeros((h, w))
        for t, i in enumerate(idx):
            y, x = divmod(i, w)
            g += 0.8 * _gauss(h, w, x + 0.6 * (u[m, t] - 0.5), y + 0.6 * (u[m, 3 - t] - 0.5), 2.2, 1.3, 0.7 + t)
        g = np.minimum(g, 0.9).astype(np.float32)
        for i in idx:
            g[i // w, i % w] = 1.0    # exactly equal maxima
        out[m] = g
    return out


DEGENERATE = ("all-zero", "all-negative", "constant", "1e-12 pixel", "1e-12 bump", "ringed", "single pixel", "zero max")


def degenerate_maps(h, w):
    out = np.zeros((len(DEGENERATE), h, w), np.float32)
    out[1] = -1.0 - 0.5 * _u("neg", h * w).reshape(h, w)       # maxval <= 0: (0, 0), no refinement
    out[2] = 0.3                                              # arg-max at index 0
    out[3, h // 2, w // 2 + 1] = 1e-12                        # every log at the clamp -> det == 0
    out[4] = 1e-12 * skewed_maps(1, h, w, "tiny")[0]           # the same with a shape the clamp hides
    cy, cx = h // 2 - 1, w // 2                               # a peak whose blurred (3 x 3) neighbours are all negative
    out[5, cy - 2:cy + 3, cx - 2:cx + 3] = -1.0
    out[5, cy - 1:cy + 2, cx - 1:cx + 2] = 0.0
    out[5, cy, cx] = 1.0
    out[6, h // 2 + 1, w // 2 - 2] = 0.7
    out[7] = np.minimum(0.0, -_u("zmax", h * w).reshape(h, w))  # max exactly 0, somewhere inside
    out[7, h // 2, w // 2] = 0.0
    return out


class Case(types.SimpleNamespace):
    """name, family, hm [S, J, h, w] fp32, ksize, center / scale [S, 2] fp32"""

    def ratio(self):
        """largest factor of the inverse crop transform: heat-map pixels -> image pixels"""
        return float(((self.scale[:, 0].astype(np.float64) * 200.0 - 1.0) / (self.hm.shape[3] - 1.0)).max())


def _case(name, family, maps, S, J, ksize):
    n, h, w = maps.shape
    assert n == S * J, (name, n, S, J)
    hm = np.ascontiguousarray(maps.reshape(S, J, h, w))
    center = (100.0 + 400.0 * _u(name + "/c", S * 2).reshape(S, 2)).astype(np.float32)
    scale = (0.5 + 1.5 * _u(name + "/s", S * 2).reshape(S, 2)).astype(np.float32)
    for a in (hm, center, scale):
        a.setflags(write=False)
    return Case(name=name, family=family, hm=hm, ksize=ksize, center=center, scale=scale)


BLUR_SIZES = (3, 5, 7, 9, 11, 17, 31)


def _build():
    cases = []
    for (h, w), sizes in (((64, 48), BLUR_SIZES + (1,)), ((20, 15), (3, 5, 7, 11))):   # (blur size 1: no blur)
        sk = skewed_maps(28, h, w, "skewed%dx%d" % (h, w))
        for k in sizes:
            if k in COMB_OF_BLUR:
                cases.append(_case("skewed-%dx%d-k%d" % (h, w, k), "skewed", np.concatenate([sk, comb_maps(h, w, k)]), 2, 15, k))
            else:
                cases.append(_case("skewed-%dx%d-k%d" % (h, w, k), "skewed", sk, 2, 14, k))
    cases.append(_case("skewed-96x72-k17", "skewed", skewed_maps(8, 96, 72, "skewed96x72"), 2, 4, 17))
    for (h, w), k in (((12, 9), 3), ((12, 9), 11), ((64, 48), 3), ((64, 48), 11)):
        cases.append(_case("guards-%dx%d-k%d" % (h, w, k), "guards", guard_maps(h, w), 2, 9, k))
    cases.append(_case("ties-64x48-k11", "ties", tie_maps(64, 48, TIES_64x48), 2, 5, 11))
    cases.append(_case("ties-96x72-k11", "ties", tie_maps(96, 72, TIES_96x72), 1, 2, 11))
    for k in (3, 11):
        cases.append(_case("degenerate-20x15-k%d" % k, "degenerate", degenerate_maps(20, 15), 2, 4, k))
    for (h, w), k, (S, J) in (((8, 6), 3, (2, 3)), ((5, 7), 3, (2, 3)), ((17, 13), 11, (2, 3)), ((128, 96), 11, (2, 2)),
                              ((160, 120), 11, (1, 4))):
        cases.append(_case("shapes-%dx%d-k%d" % (h, w, k), "shapes", skewed_maps(S * J, h, w, "shapes%dx%d" % (h, w)), S, J, k))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def expected(name, transform_back):
    """(preds [S, J, 2], maxvals [S, J, 1]) of the oracle, computed once per case and read-only"""
    c = BY_NAME[name]
    return _frozen(*post_cpu.get_final_preds(c.hm, c.center, c.scale, c.ksize, transform_back=bool(transform_back)))


@functools.lru_cache(maxsize=None)
def terms(name):
    """per map of the case, from the float64 oracle: refined [S, J] bool (the guard lets the Taylor step run), cond [S, J]
    = |det| / (|dxx dyy| + dxy^2) (nan where not refined), cross [S, J] = |dxy| / sqrt(|dxx dyy|)"""
    c = BY_NAME[name]
    coords, _ = post_cpu.get_max_preds(c.hm)
    lg = post_cpu.clamped_log(post_cpu.gaussian_blur(c.hm, c.ksize))
    S, J = c.hm.shape[:2]
    refined = np.zeros((S, J), bool)
    cond = np.full((S, J), np.nan)
    cross = np.full((S, J), np.nan)
    for s in range(S):
        for j in range(J):
            t = post_cpu.taylor_terms(lg[s, j], coords[s, j])
            if t is None:
                continue
            dx, dy, dxx, dxy, dyy = t
            refined[s, j] = True
            den = abs(dxx * dyy) + dxy ** 2
            cond[s, j] = abs(dxx * dyy - dxy ** 2) / den if den > 0 else 0.0
            cross[s, j] = abs(dxy) / np.sqrt(abs(dxx * dyy)) if dxx * dyy != 0 else np.nan
    return _frozen(refined, cond, cross)


def integer_mask(name):
    """[S, J] bool: maps whose expected coordinates are the integer arg-max position, to be met bit for bit: the guard keeps the
    Taylor step away, or the map is degenerate (zero determinant, or a zero gradient by symmetry)"""
    refined = terms(name)[0]
    return np.ones_like(refined) if BY_NAME[name].family == "degenerate" else ~refined
