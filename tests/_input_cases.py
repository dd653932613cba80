"""Scenes for the input-side kernels (csrc/i2r_input.hip: person crops and box masks) at the places where such kernels go wrong, and
two float64 models of the GEOMETRY they implement -- written from the definition of the operation (bilinear interpolation at the
exact source coordinate; indicator of a rectangle, shifted and resized), not from OpenCV's fixed-point arithmetic, so a misreading of
that arithmetic shared by the kernels and by oracle/input_cpu.py (a tap offset, a missing half pixel, the wrong odd-size shift) shows.
Used on the CPU (tests/test_input_oracle.py: the restatement against the models) and on the GPU (tests/test_input_gpu.py).

A case is an image, an output size (W, H), a rotation, a channel swap and a list of persons (centre, scale, box).  Families:
  rot0    every image size x every output size, all persons(), through input.person_inputs
  noise   the same on white noise (every tap weight of the table counts; the bound is loose there, the restatement is not)
  rot     rotations 30, -17, 90, 180 degrees: inverse maps with off-diagonal terms, through the raw C ABI
  big     1080 x 1920, two persons at the far corner: large coordinates, row offsets beyond 2^21 bytes
  tie     an inverse map whose translation * 1024 lands on .5 in both axes (exactly: raw C ABI; as get_affine_transform solves it)
Boxes of negative width or height are OUT of scope: cv2.rectangle reorders the corners, and the datasets never produce such boxes."""
import functools
import types

import numpy as np

import input_cpu
from i2r_amd import input as inp

SIZES = ((48, 64), (17, 23))      # (W, H); 17 x 23 = 391 pixels per crop: the last workgroup of 256 threads is partial
IMAGES = ((97, 131), (96, 131), (97, 130), (64, 48), (40, 30), (1, 1), (2, 3), (7, 200))   # (ih, iw); 40 x 30: the mask is magnified
BIG = (1080, 1920)
ROTATIONS = (30.0, -17.0, 90.0, 180.0)

COORD_ERR = 1.0 / 64 + 1.0 / 1024   # pixels per axis, fixed-point warp against the exact coordinate (crop_bound)
MASK_BOUND = 1.5                     # 8-bit levels, fixed-point mask against mask_f64 (derivation there)
U32 = 2.0 ** -24                     # unit round-off of fp32


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def smooth_image(ih, iw, seed):
    """uint8 [ih, iw, 3]: per channel three sinusoids of spatial frequency <= 0.12 rad/px (amplitude <= 28 levels each) plus a ramp of
    at most 40 levels across the image, rounded to 8 bit.  Neighbouring pixels differ by a few levels (at most 3 * 28 * 0.12 + 1 ~ 11),
    so a sample displaced by a fraction of a pixel moves by a fraction of a level: the bound of crop_bound stays near its floor of 0.5."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ih, 0:iw].astype(np.float64)
    out = np.empty((ih, iw, 3))
    for c in range(3):
        v = 128.0 + 40.0 * (rng.uniform(-0.5, 0.5) * xx / max(iw - 1, 1) + rng.uniform(-0.5, 0.5) * yy / max(ih - 1, 1))
        for _ in range(3):
            k, th = rng.uniform(0.03, 0.12), rng.uniform(0, 2 * np.pi)
            v += rng.uniform(12.0, 28.0) * np.sin(k * np.cos(th) * xx + k * np.sin(th) * yy + rng.uniform(0, 2 * np.pi))
        out[..., c] = v
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def noise_image(ih, iw, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(ih, iw, 3)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(kind, ih, iw):
    return _frozen((smooth_image if kind == "smooth" else noise_image)(ih, iw, 1000 * ih + iw))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 model of the crop
# ---------------------------------------------------------------------------------------------------------------------------------
def crop_f64(img, inv_m, oh, ow):
    """Bilinear interpolation of img (uint8 [ih, iw, C]) at the exact float64 source coordinate (sx, sy) = inv_m (x, y, 1) of every
    output pixel; taps outside the image read 0.  -> (value, Gx, Gy), float64 [oh, ow, C] each, in 8-bit levels.  Gx: the largest
    absolute difference between horizontally adjacent pixels of the zero-extended image inside the 4 x 4 neighbourhood (columns
    x0 - 1 .. x0 + 2, rows y0 - 1 .. y0 + 2, (x0, y0) = floor of the coordinate) around the sample; Gy: the same vertically."""
    m = np.asarray(inv_m, dtype=np.float64).reshape(6)
    src = np.asarray(img)
    ih, iw = src.shape[:2]
    PAD = 4
    P = np.zeros((ih + 2 * PAD, iw + 2 * PAD) + src.shape[2:], dtype=np.float64)
    P[PAD:PAD + ih, PAD:PAD + iw] = src
    ys, xs = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    sx = m[0] * xs + m[1] * ys + m[2]
    sy = m[3] * xs + m[4] * ys + m[5]
    fx, fy = np.floor(sx), np.floor(sy)
    ax, ay = (sx - fx)[..., None], (sy - fy)[..., None]
    # cells further out than these have an all-zero 4 x 4 neighbourhood, like the cells they are clipped to
    x0 = np.clip(fx, -3, iw + 1).astype(np.int64) + PAD
    y0 = np.clip(fy, -3, ih + 1).astype(np.int64) + PAD
    val = ((1 - ax) * (1 - ay) * P[y0, x0] + ax * (1 - ay) * P[y0, x0 + 1] + (1 - ax) * ay * P[y0 + 1, x0] + ax * ay * P[y0 + 1, x0 + 1])
    gx = np.zeros_like(val)
    gy = np.zeros_like(val)
    for a in range(-1, 3):
        for b in range(-1, 2):
            gx = np.maximum(gx, np.abs(P[y0 + a, x0 + b + 1] - P[y0 + a, x0 + b]))
            gy = np.maximum(gy, np.abs(P[y0 + b + 1, x0 + a] - P[y0 + b, x0 + a]))
    return val, gx, gy


def crop_bound(gx, gy, coord_err=COORD_ERR):
    """|fixed-point warp - crop_f64| <= 0.5 + coord_err * (Gx + Gy) levels, coord_err = 1/64 + 1/1024 px.  Derivation:
      * The fixed-point warp samples at X / 32 with X = (rint(a 1024) + rint(b 1024) + 16) >> 5, a + b the exact coordinate: the two
        rint move the sum by at most 2 * 0.5 / 1024 = 1/1024 px, and (. + 16) >> 5 rounds to the nearest 1/32: at most 1/64 px.
      * The interpolant B of the zero-extended image is continuous and bilinear inside every cell, so along x it changes at a rate of
        at most the largest difference of two horizontally adjacent pixels of the cell's two rows, and likewise along y.  A displacement
        of less than one pixel per axis stays inside the cells next to the sample's, all of whose pixels lie in the 4 x 4
        neighbourhood; walking it along x, then along y, gives |B(displaced) - B(exact)| <= coord_err * Gx + coord_err * Gy.
      * At X / 32 the table weights (32 - fx)(32 - fy) / 1024 ... are the exact bilinear weights (multiples of 1/1024 held in 15 bits;
        the one saturated entry 32767 + 1 moves the sum by |v3 - v0| / 32768 < 2^-7 of the rounding step, never across it): nothing.
      * (acc + 2^14) >> 15 rounds to the nearest level: 0.5.
    1e-9 covers the float64 evaluation of the model itself (values <= 255, a dozen operations)."""
    return 0.5 + coord_err * (gx + gy) + 1e-9


def fp32_coord_err(inv_m32, oh, ow):
    """Coordinate error in pixels of the fp32 kernel's sx = m0 x + m1 y + m2 against the exact value of the same float32 matrix.
    Three fp32 operations round (the compiler contracts one product into the sum: m0 x, fma(m1, y, .), . + m2; x, y and the matrix
    are exact), each by at most 2^-24 of its result, and no intermediate exceeds A = |m0| (ow - 1) + |m1| (oh - 1) + |m2|: 3 * 2^-24 * A
    per axis (the larger axis is taken).  floor and the fraction sx - floor(sx) are exact in fp32."""
    m = np.abs(np.asarray(inv_m32, dtype=np.float64).reshape(-1, 2, 3))
    a = m[:, :, 0] * (ow - 1) + m[:, :, 1] * (oh - 1) + m[:, :, 2]
    return 3.0 * U32 * a.max(axis=1)


# levels: what the fp32 kernel adds to coord_err * (Gx + Gy).  Weights: 1 - ax, 1 - ay and their product round (3), the product with the
# pixel (1), three additions (3): <= 7 u of a value <= 255.  Normalisation: the constant 1/255 and its product, - mean, * (1 / std)
# (4), and, when a test maps the output back to levels, the float32 rounding of mean and of 1 / std against the float64 ones (2):
# <= 13 u of 255 together; 16 u * 255 = 2.4e-4 levels.
FP32_LEVELS = 16 * U32 * 255.0


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 model of the mask
# ---------------------------------------------------------------------------------------------------------------------------------
def _mask_axis(lo, hi, n_in, n_out, shift):
    a, b = max(int(lo), 0), min(int(hi), n_in - 1)
    ind = np.zeros(n_in)
    if a <= b:
        ind[a:b + 1] = 1.0
    if shift and n_in % 2:                    # half a pixel towards higher indices: the mean with the lower neighbour, 0 at the border
        ind = 0.5 * (ind + np.concatenate([[0.0], ind[:-1]]))
    f = (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / n_out) - 0.5
    s = np.floor(f)
    fr = f - s
    s = s.astype(np.int64)
    return (1 - fr) * ind[np.clip(s, 0, n_in - 1)] + fr * ind[np.clip(s + 1, 0, n_in - 1)]


def mask_f64(box, ih, iw, oh, ow, shift=True):
    """float64 [oh, ow] in [0, 1]: the indicator of the inclusive rectangle box = (x0, y0, x1, y1) clipped to the image, averaged with
    its left neighbour when iw is odd and with its upper neighbour when ih is odd (a zero enters at the border; rotate_bound's half
    pixel), then resized bilinearly with half-pixel centres and edge replication.  Every step is separable, so this is an outer product.

    The fixed-point mask stays within MASK_BOUND = 1.5 levels (of 255) of it.  Signed error budget, in levels:
      * the shifted mask is rounded to 8 bit: 63.75 -> 64, 127.5 -> 128, 191.25 -> 191, so -0.25 .. +0.5; the resize weights are
        non-negative and sum to 1 (c0 + c1 = 2048), so it reaches the result no larger;
      * 11-bit coefficients: c1 = rint(fr 2048) is off by at most 0.5 (+ 2^-13 from the float32 fraction), c0 by the opposite amount,
        so each axis moves the result by at most 0.5 / 2048 * 255 = 0.0625: +-0.125;
      * H >> 4 drops less than 1 of a value whose 255 levels span 255 * 128: after * b <= 2048 and >> 16 that is < 1/128 level per
        term; (b (H >> 4)) >> 16 drops less than 1 of a value in quarter levels: 0.25 per term; two terms: -0.52 .. 0;
      * (. + 2) >> 2 rounds quarter levels to the nearest level: -0.5 .. +0.5.
    Upwards at most 0.5 + 0.125 + 0.5 = 1.125, downwards at most 0.25 + 0.125 + 0.52 + 0.5 = 1.395: both below 1.5."""
    x0, y0, x1, y1 = [int(v) for v in box]
    return np.outer(_mask_axis(y0, y1, ih, oh, shift), _mask_axis(x0, x1, iw, ow, shift))


# ---------------------------------------------------------------------------------------------------------------------------------
# persons and cases
# ---------------------------------------------------------------------------------------------------------------------------------
def persons(ih, iw):
    """name -> box (x, y, w, h) in the dataset convention, for an image of ih x iw"""
    bw, bh = max(0.4 * iw, 2.0), max(0.5 * ih, 2.0)
    far = 10.0 * max(bw, bh) + 50.0
    return dict([
        ("interior", (0.3 * iw, 0.25 * ih, bw, bh)),
        ("left", (-0.5 * bw, 0.25 * ih, bw, bh)),                  # half of the person outside, one side each
        ("right", (iw - 0.5 * bw, 0.25 * ih, bw, bh)),
        ("top", (0.3 * iw, -0.5 * bh, bw, bh)),
        ("bottom", (0.3 * iw, ih - 0.5 * bh, bw, bh)),
        ("outside-", (-far, -far, bw, bh)),                       # the whole crop outside: source coordinates far below zero ...
        ("outside+", (iw + far, ih + far, bw, bh)),               # ... and far beyond the last pixel; the rectangle clips to nothing
        ("larger", (-0.5 * iw, -0.5 * ih, 2.0 * iw, 2.0 * ih)),   # strong minification; the mask is 1 up to the odd-size shift
        ("thin", (0.5 * iw - 1.5, 0.5 * ih - 2.0, 3.0, 4.0)),     # 3.75 px across W outputs: 17x at W = 48, many outputs per source cell
        ("w0", (0.5 * iw, 0.2 * ih, 0.0, max(0.6 * ih, 3.0))),    # inclusive corners: a line one pixel wide
        ("h0", (0.2 * iw, 0.5 * ih, max(0.6 * iw, 3.0), 0.0)),
    ])


ALL = tuple(persons(1, 1))
OUTSIDE = ("outside-", "outside+")
ROTATED = ("interior", "left", "bottom", "larger", "thin")


class Case(types.SimpleNamespace):
    """name, family, kind, ih, iw, size = (W, H), rot, swap_rb, who (person names), centers / scales [n, 2] fp32, boxes [n, 4] f64,
    forward: None, or [n, 2, 3] forward maps given directly instead of get_affine_transform(centers, scales, rot, size)"""

    @property
    def img(self):
        return image(self.kind, self.ih, self.iw)

    @property
    def n(self):
        return len(self.who)

    @property
    def raw(self):
        """the case cannot go through input.person_inputs (which builds the maps itself, at rot = 0): raw C ABI"""
        return self.rot != 0 or self.forward is not None

    def trans(self):
        """[n, 2, 3] float64: the forward maps the reference hands to cv2.warpAffine"""
        if self.forward is not None:
            return self.forward
        return np.stack([inp.get_affine_transform(self.centers[i], self.scales[i], self.rot, self.size) for i in range(self.n)])

    def inv(self):
        """[n, 6] float64: the inverse maps cv2.warpAffine derives from them"""
        return np.stack([inp.cv2_inverse(t) for t in self.trans()]).reshape(self.n, 6)

    def inv32(self):
        """[n, 6] float32: what the fp32 kernel receives (input.person_inputs(fixed_point=False) builds it this way at rot = 0)"""
        return np.stack([inp.invert_affine(t) for t in self.trans()]).reshape(self.n, 6).astype(np.float32)

    def boxes_int(self):
        """inclusive integer corners, as cv2.rectangle gets them (JointsDataset.py:168-169)"""
        return [(int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])) for b in self.boxes]


def _case(name, family, kind, ih, iw, size, rot, swap_rb, who, boxes=None, centers=None, scales=None, forward=None):
    if boxes is None:
        table = persons(ih, iw)
        boxes = [table[w] for w in who]
    boxes = np.asarray(boxes, dtype=np.float64).reshape(len(who), 4)
    if centers is None:
        cs = [inp.box_to_center_scale(b, size) for b in boxes]
        centers, scales = np.stack([c for c, _ in cs]), np.stack([s for _, s in cs])
    centers, scales = np.asarray(centers, dtype=np.float32), np.asarray(scales, dtype=np.float32)
    _frozen(boxes, centers, scales)
    return Case(name=name, family=family, kind=kind, ih=ih, iw=iw, size=tuple(size), rot=float(rot), swap_rb=bool(swap_rb), who=tuple(who),
                boxes=boxes, centers=centers, scales=scales, forward=forward)


# The tie: W = 17 and scale 9 / 200 give src_w = 9, so the forward map is (dst_w - 1) / (src_w - 1) = 16 / 8 = 2 and the inverse has
# m0 = m4 = 0.5; with rot = 0, m1 = m3 = 0.  The centre (10 + 1/2048, 20.5 + 3/2048) is exact in float32, and m2 = cx - 0.5 * 8 =
# 6 + 1/2048, m5 = cy - 0.5 * 11 = 15 + 3/2048, so m2 * 1024 = 6144.5 and m5 * 1024 = 15361.5: ties, one between an even and an odd
# integer each way round.  rint(m0 x 1024) = 512 x is exact.  The kernel's llrint rounds in the current (default) mode, to nearest even,
# and so does numpy's rint in the restatement: 6144 (half away from zero: 6145) and 15362 (truncation: 15361).  The 3 x 3 solve of
# get_affine_transform returns these entries only to an ulp (m1 = 5e-17, m4 = 0.5 + 1e-16: some rows tie, some do not), so the case
# "tie-exact" hands the kernel the exact forward map [[2, 0, -2 m2], [0, 2, -2 m5]] -- whose closed-form inverse is exact: D = 1/4,
# 2 * (1/4) = 0.5, 0.5 * (2 m2) = m2 -- through the raw C ABI, and "tie-solved" keeps the solved one.
#
# Those two ties do not reach a pixel: after + 16 and >> 5 both 6144 and 6145 fall into the same 1/32 cell.  A tie decides a pixel
# only next to a cell boundary, X0 = 15.5 (mod 32).  There nearest-even, half-up and half-away agree for a positive coordinate (15 is
# odd) and differ from truncation; for a negative one, -16.5, nearest-even gives -16 and half-away-from-zero -17.  "tie-deciding" has
# both: m2 * 1024 = 6144 + 15.5 -> 6160, (6160 + 16) >> 5 = 193 (truncation: 192), and m5 * 1024 = -16.5 -> -16, (-16 + 16) >> 5 = 0:
# output row 0 is source row 0 (half away from zero: -1 >> 5 = -1, source row -1/32 -- almost all border).
TIE_CENTER = (10.0 + 1.0 / 2048, 20.5 + 3.0 / 2048)
TIE_SCALE = (9.0 / 200.0, 9.0 / 200.0 * 23.0 / 17.0)
TIE_INV = (0.5, 0.0, 6.0 + 1.0 / 2048, 0.0, 0.5, 15.0 + 3.0 / 2048)
TIE2_INV = (0.5, 0.0, 6.0 + 31.0 / 2048, 0.0, 0.5, -33.0 / 2048)


def tie_forward(inv_m):
    """the forward map whose closed-form inverse (cv2_inverse) is exactly the uniform 1/2 scale inv_m"""
    return np.array([[[2.0, 0.0, -2.0 * inv_m[2]], [0.0, 2.0, -2.0 * inv_m[5]]]])


def _build():
    cases = []
    for i, (ih, iw) in enumerate(IMAGES):
        for j, size in enumerate(SIZES):
            cases.append(_case("rot0-%dx%d-%dx%d" % (ih, iw, size[0], size[1]), "rot0", "smooth", ih, iw, size, 0, (i + j) % 2, ALL))
    for i, (ih, iw) in enumerate(((97, 131), (40, 30))):
        for j, size in enumerate(SIZES):
            cases.append(_case("noise-%dx%d-%dx%d" % (ih, iw, size[0], size[1]), "noise", "noise", ih, iw, size, 0, (i + j + 1) % 2, ALL))
    for i, rot in enumerate(ROTATIONS):
        for j, size in enumerate(SIZES):
            cases.append(_case("rot%+d-97x131-%dx%d" % (rot, size[0], size[1]), "rot", "smooth", 97, 131, size, rot, (i + j) % 2, ROTATED))
    cases.append(_case("rot+30-noise-64x48-17x23", "rot", "noise", 64, 48, SIZES[1], 30.0, 1, ROTATED))
    cases.append(_case("rot-17-noise-96x131-48x64", "rot", "noise", 96, 131, SIZES[0], -17.0, 0, ROTATED))
    ih, iw = BIG
    far = [(1700.0, 880.0, 150.0, 170.0), (1850.0, 1000.0, 120.0, 140.0)]   # the second sticks out of the far corner
    for j, size in enumerate(SIZES):
        cases.append(_case("big-%dx%d-%dx%d" % (ih, iw, size[0], size[1]), "big", "smooth", ih, iw, size, 0, j, ("far", "corner"), boxes=far))
    cases.append(_case("big-rot+30-%dx%d-48x64" % (ih, iw), "big", "smooth", ih, iw, SIZES[0], 30.0, 1, ("far", "corner"), boxes=far))
    for name, forward in (("tie-solved", None), ("tie-exact", tie_forward(TIE_INV)), ("tie-deciding", tie_forward(TIE2_INV))):
        cases.append(_case(name + "-97x131-17x23", "tie", "smooth", 97, 131, SIZES[1], 0, 0, ("tie",), boxes=[(8.0, 15.0, 5.0, 11.0)],
                           centers=[TIE_CENTER], scales=[TIE_SCALE], forward=forward))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def restated(name):
    """oracle/input_cpu.py on the case, computed once and read-only: (crop levels uint8 [n, 3, H, W], mask levels uint8 [n, H, W])"""
    c = BY_NAME[name]
    W, H = c.size
    src = c.img[:, :, ::-1] if c.swap_rb else c.img
    crops = np.stack([input_cpu.cv2_warp_affine(src, t, (W, H)).transpose(2, 0, 1) for t in c.trans()])
    m = input_cpu.box_mask_cv2(c.boxes_int(), c.ih, c.iw, H, W)[:, 0]
    levels = np.rint(m.astype(np.float64) * 255.0)
    assert np.array_equal(levels.astype(np.float32) * np.float32(1.0 / 255.0), m)   # (level * fp32(1 / 255): the level is recoverable)
    return _frozen(np.ascontiguousarray(crops), levels.astype(np.uint8))


@functools.lru_cache(maxsize=None)
def modelled(name, fp32=False):
    """the float64 models on the case, computed once and read-only: (crop value, Gx + Gy) [n, 3, H, W] in levels, mask [n, H, W] in
    levels.  fp32: the crop at the float32-rounded inverse maps and the mask without the odd-size shift (what the fp32 kernels do)."""
    c = BY_NAME[name]
    W, H = c.size
    src = c.img[:, :, ::-1] if c.swap_rb else c.img
    val, g = [], []
    for m in (c.inv32() if fp32 else c.inv()):
        v, gx, gy = crop_f64(src, m, H, W)
        val.append(v.transpose(2, 0, 1))
        g.append((gx + gy).transpose(2, 0, 1))
    mask = np.stack([mask_f64(b, c.ih, c.iw, H, W, shift=not fp32) for b in c.boxes_int()]) * 255.0
    return _frozen(np.stack(val), np.stack(g), mask)


def levels_of(x, mean=inp.IMAGENET_MEAN, std=inp.IMAGENET_STD):
    """normalised fp32 [n, 3, H, W] -> (x std + mean) 255 in float64, unrounded: the 8-bit level a fixed-point kernel produced is rint of it"""
    x = np.asarray(x, dtype=np.float64)
    return (x * np.asarray(std, dtype=np.float64)[None, :, None, None] + np.asarray(mean, dtype=np.float64)[None, :, None, None]) * 255.0


def zero_level(mean=inp.IMAGENET_MEAN, std=inp.IMAGENET_STD):
    """[3] fp32: (0 - mean) / std as the kernels round it -- fp32 mean, fp32 (1 / std), one fp32 product"""
    return (-np.asarray(mean, dtype=np.float32)) * np.asarray([1.0 / s for s in std], dtype=np.float32)
