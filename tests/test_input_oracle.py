"""CPU: host logic of the input side (i2r_amd/input.py) and its CPU restatement (oracle/input_cpu.py).  collate() is pinned by a
fixture the reference's own collater produced (oracle/make_golden_collate.py); the cv2 steps are held to float64 models of their
geometry (tests/_input_cases.py); cv2's own rounding choices stay unpinned (cv2 absent)."""
import os

import numpy as np
import pytest
import torch

import _input_cases as ic
import input_cpu
from i2r_amd import input as inp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_collate_matches_reference_collater_fixture():
    g = np.load(os.path.join(GOLDEN, "collate.npz"))
    persons = g["persons"].tolist()
    batch, o = [], 0
    for n in persons:
        batch.append(([torch.from_numpy(g["inputs"][o + i]) for i in range(n)], [torch.from_numpy(g["masks"][o + i]) for i in range(n)]))
        o += n
    x, m, length = inp.collate(batch)
    assert length == g["out_length"].tolist() == persons
    assert np.array_equal(x.numpy(), g["out_x"]) and np.array_equal(m.numpy(), g["out_m"])
    # stacked per-image tensors are accepted as well
    x2, m2, l2 = inp.collate([(torch.stack(a), torch.stack(b)) for a, b in batch])
    assert torch.equal(x2, x) and torch.equal(m2, m) and l2 == length


def test_affine_transform_geometry():
    """rot = 0: a uniform scale (dst_w-1)/(scale*200-1) about the centres (transforms.py:61-96); inverse flag and invert agree."""
    c, s, size = np.array([310.5, 222.25]), np.array([1.3, 1.3 * 256 / 192]), (192, 256)
    t = inp.get_affine_transform(c, s, 0, size)
    k = (size[0] - 1) / (s[0] * 200.0 - 1)
    assert np.allclose(t[:, :2], np.eye(2) * k, atol=1e-5)
    assert np.allclose(t @ np.array([c[0], c[1], 1.0]), [(size[0] - 1) * 0.5, (size[1] - 1) * 0.5], atol=1e-3)
    ti = inp.get_affine_transform(c, s, 0, size, inv=1)
    assert np.allclose(inp.invert_affine(t), ti, atol=1e-4)
    r = inp.get_affine_transform(c, s, 30, size)
    assert np.allclose(np.linalg.det(r[:, :2]), k * k, rtol=1e-4)


def test_oracle_crop_identity_and_border():
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(9, 7, 3)).astype(np.uint8)
    ident = np.array([[[1, 0, 0], [0, 1, 0]]], dtype=np.float32)
    out = input_cpu.crop_affine(img, ident, (0, 0, 0), (1, 1, 1), 9, 7)
    assert np.allclose(out[0], img.transpose(2, 0, 1) / 255.0, atol=1e-6)
    shift = np.array([[[1, 0, -2.5], [0, 1, 0]]], dtype=np.float32)   # samples 2.5 px left of the image: columns 0..1 see the border
    out = input_cpu.crop_affine(img, shift, (0, 0, 0), (1, 1, 1), 9, 7)
    assert np.all(out[0][:, :, :2] == 0) and np.allclose(out[0][:, :, 2], 0.5 * img[:, 0].T / 255.0, atol=1e-6)
    bgr = input_cpu.crop_affine(img, ident, (0, 0, 0), (1, 1, 1), 9, 7, swap_rb=True)
    assert np.allclose(bgr[0], img[:, :, ::-1].transpose(2, 0, 1) / 255.0, atol=1e-6)


def test_oracle_box_mask():
    m = input_cpu.box_mask([(2, 3, 5, 6)], 8, 8, 8, 8)   # no resize: the inclusive rectangle itself
    ref = np.zeros((8, 8), dtype=np.float32)
    ref[3:7, 2:6] = 1
    assert np.array_equal(m[0, 0], ref)
    m2 = input_cpu.box_mask([(0, 0, 99, 49)], 50, 100, 25, 50)
    assert np.all(m2 == 1.0)
    m3 = input_cpu.box_mask([(11, 10, 58, 39)], 100, 200, 50, 100)   # 2x down-scale, odd edges: half-covered samples on the rim
    assert m3.min() == 0 and m3.max() == 1 and ((m3 > 0) & (m3 < 1)).any()


def test_cv2_fixed_point_restatement_known_answers():
    """oracle/input_cpu.py's restatement of cv2's fixed-point warp / resize (parity unpinned: cv2 absent) on cases whose answer follows
    from the published algorithm alone: table sums, identity warp, half-pixel shift = rounded mean of neighbours, identity resize,
    rotate_bound's shift only for odd dimensions."""
    tab = input_cpu.cv2_bilinear_tab()
    assert tab.shape == (32, 32, 4) and (tab.sum(-1) == 1 << 15).all() and list(tab[16, 16]) == [8192] * 4
    img = np.random.RandomState(0).randint(0, 256, (60, 81, 3)).astype(np.uint8)
    assert np.array_equal(input_cpu.cv2_warp_affine(img, np.array([[1.0, 0, 0], [0, 1.0, 0]]), (81, 60)), img)
    half = input_cpu.cv2_warp_affine(img, np.array([[1.0, 0, 0.5], [0, 1.0, 0]]), (81, 60))
    assert np.array_equal(half[:, 1:].astype(int), (img[:, :-1].astype(int) + img[:, 1:].astype(int) + 1) >> 1)
    assert (half[:, 0].astype(int) == (img[:, 0].astype(int) + 1) >> 1).all()       # the left tap is outside: border value 0
    m = np.zeros((61, 81), np.uint8)
    m[10:40, 20:50] = 255
    assert np.array_equal(input_cpu.cv2_resize_linear_u8(m, (81, 61)), m)
    even = input_cpu.box_mask_cv2([(20, 10, 49, 39)], 60, 80, 60, 80)[0, 0]
    assert set(np.unique(even)) == {0.0, 1.0} and even[10:40, 20:50].min() == 1.0   # even size, same size: the rectangle itself
    odd = input_cpu.box_mask_cv2([(20, 10, 49, 39)], 61, 81, 61, 81)[0, 0]
    assert abs(odd[25, 20] - 128 / 255) < 1e-6 and odd[25, 21] == 1.0 and abs(odd[10, 30] - 128 / 255) < 1e-6  # edges blurred by the 0.5 px shift


# ---- the restatement against float64 models of the geometry (tests/_input_cases.py) ----
def _crop_violations(levels, value, g):
    return int((np.abs(levels.astype(np.float64) - value) > ic.crop_bound(g, 0.0)).sum())


@pytest.mark.parametrize("name", ic.NAMES)
def test_restatement_within_float64_geometry(name):
    """oracle/input_cpu.py's fixed-point warp and mask over the whole case list: every crop pixel within 0.5 + (1/64 + 1/1024)(Gx + Gy)
    levels of the bilinear interpolation at the exact coordinate (ic.crop_bound), every mask pixel within 1.5 levels of the shifted and
    resized indicator (ic.mask_f64) -- no pixel is left out.  Measured: worst crop deviation 0.999 of its bound (a value on .5 in a flat
    region, rounded up), median bound 0.53 levels on the smooth images; worst mask deviation 0.90 levels (2 x 3 image)."""
    c = ic.BY_NAME[name]
    levels, mask = ic.restated(name)
    value, g, mask64 = ic.modelled(name)
    assert levels.shape == value.shape == (c.n, 3, c.size[1], c.size[0]) and mask.shape == mask64.shape == (c.n, c.size[1], c.size[0])
    dev = np.abs(levels.astype(np.float64) - value) / ic.crop_bound(g, 0.0)
    mdev = np.abs(mask.astype(np.float64) - mask64)
    print("%s: crop worst %.3f of its bound (median bound %.2f levels), mask worst %.3f levels" % (name, dev.max(), np.median(ic.crop_bound(g, 0.0)), mdev.max()))
    assert _crop_violations(levels, value, g) == 0
    assert mdev.max() <= ic.MASK_BOUND
    for k, who in enumerate(c.who):
        if who in ic.OUTSIDE:    # the whole crop outside the image: border value 0 everywhere, and a rectangle that clips to nothing
            assert (levels[k] == 0).all() and (mask[k] == 0).all() and (value[k] == 0).all() and (mask64[k] == 0).all()
        if who == "larger":      # the mask of a box larger than the image: 1 except the first row / column of an odd dimension, halved
            ref = np.outer(np.where((np.arange(c.size[1]) + 0.5) * c.ih / c.size[1] - 0.5 < 1, np.nan, 1.0) if c.ih % 2 else np.ones(c.size[1]),
                           np.where((np.arange(c.size[0]) + 0.5) * c.iw / c.size[0] - 0.5 < 1, np.nan, 1.0) if c.iw % 2 else np.ones(c.size[0]))
            ok = ~np.isnan(ref)  # (outputs that touch source row / column 0 of an odd dimension are left to the bound above)
            assert (mask[k][ok] == 255).all() and (mask64[k][ok] == 255.0).all()


def test_float64_crop_bound_has_teeth():
    """the crop bound tells a restatement whose inverse map is off by 1/8 px or by 1 px from a correct one (97 x 131 smooth image,
    rotation 0, the interior person at 48 x 64: 9216 values; measured along x / y: 0 / 0, then 1010 / 1369 and 7198 / 7341 violations)"""
    c = ic.BY_NAME["rot0-97x131-48x64"]
    k = c.who.index("interior")
    W, H = c.size
    src = c.img[:, :, ::-1] if c.swap_rb else c.img
    levels = ic.restated(c.name)[0][k]
    counts = []
    for d in (0.0, 1.0 / 8, 1.0):
        for axis in (2, 5):
            m = c.inv()[k].copy()
            m[axis] += d
            v, gx, gy = ic.crop_f64(src, m, H, W)
            counts.append(_crop_violations(levels, v.transpose(2, 0, 1), (gx + gy).transpose(2, 0, 1)))
    print("violations of %d at 0, 1/8, 1 px (x, y each):" % levels.size, counts)
    assert levels.size == 9216 and counts[0] == counts[1] == 0
    assert all(n > 0 for n in counts[2:])


def test_float64_models_known_answers():
    """the models themselves, on cases whose answer follows from the definition"""
    img = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3) * 4
    v, gx, gy = ic.crop_f64(img, (1, 0, 0, 0, 1, 0), 5, 4)                       # identity
    assert np.array_equal(v, img.astype(np.float64))
    assert gx[2, 1, 0] == 12 and gy[2, 1, 0] == 48 and gx[2, 0, 0] == img[1:5, 0, 0].max()   # (the last: the border's step)
    v, _, _ = ic.crop_f64(img, (1, 0, 0.25, 0, 1, -0.5), 5, 4)                    # (x + 1/4, y - 1/2): the top row sees half a border row
    assert v[0, 0, 0] == 0.5 * (0.75 * img[0, 0, 0] + 0.25 * img[0, 1, 0]) and v[1, 3, 1] == 0.75 * 0.5 * (float(img[0, 3, 1]) + img[1, 3, 1])
    v, _, _ = ic.crop_f64(img, (0, -1, 4, 1, 0, 0), 4, 5)                         # a quarter turn: (x, y) <- (4 - y, x)
    assert v[0, 0, 0] == 0 and v[1, 0, 0] == img[0, 3, 0] and v[1, 2, 0] == img[2, 3, 0] and v[3, 4, 0] == img[4, 1, 0]
    m = ic.mask_f64((1, 1, 2, 3), 6, 4, 6, 4)                                     # even size, no resize: the rectangle itself
    ref = np.zeros((6, 4))
    ref[1:4, 1:3] = 1
    assert np.array_equal(m, ref)
    m = ic.mask_f64((1, 1, 2, 3), 5, 4, 5, 4)                                     # odd height: averaged with the row above
    assert np.array_equal(m[:, 1], [0, 0.5, 1, 1, 0.5]) and np.array_equal(m[:, 0], np.zeros(5))
    assert np.array_equal(ic.mask_f64((1, 1, 2, 3), 5, 4, 5, 4, shift=False)[:, 1], [0, 1, 1, 1, 0])
    m = ic.mask_f64((0, 0, 3, 0), 2, 4, 4, 8)                                     # 2x magnification: quarter steps, replicated edges
    assert np.array_equal(m[:, 3], [1, 0.75, 0.25, 0]) and np.array_equal(m[0], np.ones(8))
    assert not ic.mask_f64((4, 0, 9, 1), 2, 4, 4, 8).any() and not ic.mask_f64((-5, -5, -1, 1), 2, 4, 4, 8).any()   # clipped to nothing


def test_tie_cases_are_ties_and_round_half_to_even():
    c = ic.BY_NAME["tie-exact-97x131-17x23"]
    assert np.array_equal(c.inv()[0], np.array(ic.TIE_INV))                       # the closed-form inverse of the forward map is exact
    assert (ic.TIE_INV[2] * 1024, ic.TIE_INV[5] * 1024) == (6144.5, 15361.5)
    assert np.abs(ic.BY_NAME["tie-solved-97x131-17x23"].inv()[0] - np.array(ic.TIE_INV)).max() < 1e-14   # the solve: the same map to an ulp
    c = ic.BY_NAME["tie-deciding-97x131-17x23"]
    assert np.array_equal(c.inv()[0], np.array(ic.TIE2_INV))
    assert (ic.TIE2_INV[2] * 1024, ic.TIE2_INV[5] * 1024) == (6144 + 15.5, -16.5)
    e = 2.0 ** -30

    def warp(dx, dy):   # the map whose exact inverse translation is (m2 + dx, m5 + dy)
        return input_cpu.cv2_warp_affine(c.img, ic.tie_forward((0.5, 0, ic.TIE2_INV[2] + dx, 0, 0.5, ic.TIE2_INV[5] + dy))[0], c.size)
    tie = ic.restated(c.name)[0][0].transpose(1, 2, 0)
    assert np.array_equal(tie, warp(+e, +e))                                      # 6159.5 -> 6160 (up), -16.5 -> -16 (up): to even
    assert not np.array_equal(tie, warp(-e, +e)) and not np.array_equal(tie, warp(+e, -e))   # and each tie decides pixels
    assert np.array_equal(tie[0, 0], c.img[0, 6] + ((c.img[0, 7].astype(int) - c.img[0, 6]) * 1 + 16) // 32)   # row 0 at column 6 + 1/32


def test_cv2_restatement_known_answers_at_the_new_edges():
    """1 x 1 and 2 x 3 images, a rectangle that clips to nothing, a crop entirely outside the image"""
    one = np.array([[[200, 100, 7]]], dtype=np.uint8)
    out = input_cpu.cv2_warp_affine(one, np.array([[1.0, 0, 1.0], [0, 1.0, 1.0]]), (3, 3))     # the pixel lands on (1, 1), border elsewhere
    ref = np.zeros((3, 3, 3), np.uint8)
    ref[1, 1] = one[0, 0]
    assert np.array_equal(out, ref)
    half = input_cpu.cv2_warp_affine(one, np.array([[1.0, 0, 0.5], [0, 1.0, 0.5]]), (2, 2))     # a quarter of it on four outputs, rounded
    assert np.array_equal(half, np.broadcast_to((one[0, 0].astype(int) * 8192 + 16384) >> 15, (2, 2, 3)))
    # masks: 1 x 1 is odd both ways -> the covered pixel becomes (255 * 8192 + 16384) >> 15 = 64, replicated over any output
    assert np.array_equal(input_cpu.box_mask_cv2([(0, 0, 0, 0)], 1, 1, 5, 4)[0, 0], np.full((5, 4), np.float32(64) * np.float32(1 / 255.0)))
    # 2 x 3 (odd width): the full rectangle shifts to rows (128, 255, 255); same size: unchanged; twice the width: 1/4 steps between taps
    full = input_cpu.box_mask_cv2([(-1, -1, 9, 9)], 2, 3, 2, 3)[0, 0]
    assert np.array_equal(np.rint(full * 255), [[128, 255, 255]] * 2)
    wide = np.rint(input_cpu.box_mask_cv2([(-1, -1, 9, 9)], 2, 3, 2, 6)[0, 0] * 255)
    assert np.array_equal(wide, [[128, 160, 223, 255, 255, 255]] * 2)            # 128 + 127 / 4 = 159.75, 128 + 127 * 3 / 4 = 223.25
    line = np.rint(input_cpu.box_mask_cv2([(1, 0, 1, 1)], 2, 3, 2, 3)[0, 0] * 255)   # a one-pixel column (w = 0): half of it moves right
    assert np.array_equal(line, [[0, 128, 128]] * 2)
    for box in ((-10, -10, -1, 5), (3, 0, 8, 1), (0, 2, 2, 9), (0, -7, 2, -1)):   # clip to nothing on each side
        assert not input_cpu.box_mask_cv2([box], 2, 3, 7, 5).any()
    img = np.full((9, 7, 3), 255, np.uint8)
    far = np.array([[[1.0, 0, 500.0], [0, 1.0, 0]], [[1.0, 0, 0], [0, 1.0, -9.0]], [[0.5, 0, -4000.25], [0, 0.5, -3000.5]]])
    out = input_cpu.crop_affine_cv2(img, far, inp.IMAGENET_MEAN, inp.IMAGENET_STD, 9, 7)
    assert np.array_equal(out, np.broadcast_to(ic.zero_level()[None, :, None, None], out.shape))
    near = input_cpu.cv2_warp_affine(img, np.array([[1.0, 0, 7.0 - 1 / 64], [0, 1.0, 0]]), (7, 9))   # 1/64 px from leaving: rounds up to 1/32 px
    assert (near[:, :6] == 0).all() and (near[:, 6] == (255 * 1 * 32 * 32 + 16384) >> 15).all()      # (-63/64 -> cell -1, fraction 1/32: 8)
