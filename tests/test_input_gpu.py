"""-m gpu: the input-side kernels (csrc/i2r_input.hip) through the C-ABI against the CPU restatement of the same definition and, over
the scenes of tests/_input_cases.py, against float64 models of the geometry; and the whole chain image -> crops -> forward."""
import ctypes as C

import numpy as np
import pytest
import torch

import _input_cases as ic
import input_cpu
from _golden import setup
from i2r_amd import cabi
from i2r_amd import input as inp
from i2r_amd import models

pytestmark = pytest.mark.gpu


def _scene(seed, ih, iw, n):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, size=(ih, iw, 3)).astype(np.uint8)
    boxes = []
    for _ in range(n):
        w, h = rng.uniform(0.15, 0.6) * iw, rng.uniform(0.2, 0.8) * ih
        x, y = rng.uniform(-0.1 * iw, iw - 0.5 * w), rng.uniform(-0.1 * ih, ih - 0.5 * h)   # some boxes stick out of the image
        boxes.append((x, y, w, h))
    centers = [np.array([b[0] + b[2] * 0.5, b[1] + b[3] * 0.5]) for b in boxes]
    scales = []
    for b in boxes:   # _box2cs convention of the datasets: aspect-corrected box / 200 * 1.25
        w, h = b[2], b[3]
        if w > 0.75 * h:
            h = w / 0.75
        else:
            w = h * 0.75
        scales.append(np.array([w / 200.0, h / 200.0]) * 1.25)
    return img, centers, scales, boxes


@pytest.mark.parametrize("ih,iw,n,rgb", [(480, 640, 3, False), (333, 517, 2, True), (64, 48, 1, False)])
def test_crops_and_masks_match_cpu_restatement(ih, iw, n, rgb):
    img, centers, scales, boxes = _scene(ih + n, ih, iw, n)
    x, m = inp.person_inputs(img, centers, scales, boxes, (192, 256), color_rgb=rgb, fixed_point=False)
    torch.cuda.synchronize()
    inv = np.stack([inp.invert_affine(inp.get_affine_transform(centers[i], scales[i], 0, (192, 256))) for i in range(n)]).astype(np.float32)
    ref_x = input_cpu.crop_affine(img, inv, inp.IMAGENET_MEAN, inp.IMAGENET_STD, 256, 192, swap_rb=rgb)
    bx = [(int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])) for b in boxes]
    ref_m = input_cpu.box_mask(bx, ih, iw, 256, 192)
    assert x.shape == (n, 3, 256, 192) and m.shape == (n, 1, 256, 192)
    # fp32 bilinear on both sides; contraction order of the four taps may differ by an ulp of a 0..255 value
    assert np.abs(x.cpu().numpy() - ref_x).max() < 2e-4
    assert np.abs(m.cpu().numpy() - ref_m).max() < 1e-6


@pytest.mark.parametrize("ih,iw,n,rgb", [(480, 640, 3, False), (333, 517, 2, True), (64, 48, 1, False), (121, 90, 2, False)])
def test_crops_and_masks_cv2_fixed_point(ih, iw, n, rgb):
    """the default mode: cv2's fixed-point arithmetic (1/32-pixel grid, 15-bit weights, 8-bit results; masks of odd-sized images shifted
    by half a pixel like rotate_bound does) -- integer arithmetic, so the kernel must agree with the numpy restatement EXACTLY"""
    img, centers, scales, boxes = _scene(ih + n, ih, iw, n)
    x, m = inp.person_inputs(img, centers, scales, boxes, (192, 256), color_rgb=rgb)
    torch.cuda.synchronize()
    trans = np.stack([inp.get_affine_transform(centers[i], scales[i], 0, (192, 256)) for i in range(n)])
    ref_x = input_cpu.crop_affine_cv2(img, trans, inp.IMAGENET_MEAN, inp.IMAGENET_STD, 256, 192, swap_rb=rgb)
    bx = [(int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])) for b in boxes]
    ref_m = input_cpu.box_mask_cv2(bx, ih, iw, 256, 192)
    # same 8-bit level everywhere (one level = 1/255/std ~ 0.017); the float normalisation may differ in the last bit
    assert np.abs(x.cpu().numpy() - ref_x).max() < 1e-5
    assert np.array_equal(m.cpu().numpy(), ref_m)
    # and it is close to the fp32 interpolation of the same geometry (half an intensity level + 1/64 pixel)
    x32, m32 = inp.person_inputs(img, centers, scales, boxes, (192, 256), color_rgb=rgb, fixed_point=False)
    assert (x - x32).abs().mean().item() < 0.02


def test_person_inputs_batch_is_bit_identical_to_per_image_path():
    """input.person_inputs_batch (ONE launch + ONE table upload for all persons of all images of a batch, images of different sizes)
    writes exactly what person_inputs per image + collate produce, and hands centres / scales over as device tensors"""
    scenes = [_scene(11, 240, 320, 3), _scene(12, 333, 517, 1), _scene(13, 121, 90, 2)]
    per_image = [inp.person_inputs(*sc, (192, 256), color_rgb=True) for sc in scenes]
    x_ref, m_ref, len_ref = inp.collate(per_image)
    imgs = [torch.from_numpy(sc[0]).cuda() for sc in scenes]
    x, m, length, cen, scl = inp.person_inputs_batch(imgs, [sc[1] for sc in scenes], [sc[2] for sc in scenes], [sc[3] for sc in scenes],
                                                     (192, 256), color_rgb=True)
    torch.cuda.synchronize()
    assert length == len_ref == [3, 1, 2]
    assert torch.equal(x, x_ref) and torch.equal(m, m_ref)
    assert np.array_equal(cen.cpu().numpy(), np.concatenate([np.stack(sc[1]) for sc in scenes]).astype(np.float32))
    assert np.array_equal(scl.cpu().numpy(), np.concatenate([np.stack(sc[2]) for sc in scenes]).astype(np.float32))


def test_person_inputs_malformed_crop_table_writes_zeros():
    """raw C-ABI: a crop whose image index lies outside the image table (device memory the host entry point cannot validate) gets zero
    rows instead of an out-of-bounds read, and so does one whose image entry is empty (null pointer, ih = 0, iw = 0); the well-formed
    crops around them are untouched (include/i2r_hip.h, i2r_person_inputs_cv2).  Every malformed crop returns before any image read."""
    img, centers, scales, boxes = _scene(21, 120, 160, 2)
    im = torch.from_numpy(img).cuda()
    x_ref, m_ref, _, _, _ = inp.person_inputs_batch([im], [centers], [scales], [boxes], (192, 256))
    tab = x_ref._i2r_keep[0].clone()          # [crop table (2 x 80 bytes) | image table | ...]
    tab_h = tab.cpu()
    tab_h.numpy()[:160].view(inp._CROP_DT)["image"][1] = 7   # only one image in the table
    tab = tab_h.cuda()
    x = torch.full_like(x_ref, 5.0)
    m = torch.full_like(m_ref, 5.0)
    mean_c = (C.c_float * 3)(*inp.IMAGENET_MEAN)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in inp.IMAGENET_STD])
    st = torch.cuda.current_stream().cuda_stream
    cabi.check(cabi.lib().i2r_person_inputs_cv2(tab.data_ptr() + 160, 1, tab.data_ptr(), 2, 0, mean_c, istd_c, x.data_ptr(), m.data_ptr(), 256, 192, st),
               "i2r_person_inputs_cv2")
    torch.cuda.synchronize()
    assert torch.equal(x[0], x_ref[0]) and torch.equal(m[0], m_ref[0])
    assert (x[1] == 0).all() and (m[1] == 0).all()
    assert cabi.lib().i2r_person_inputs_cv2(tab.data_ptr() + 160, 0, tab.data_ptr(), 2, 0, mean_c, istd_c, x.data_ptr(), m.data_ptr(), 256, 192, st) == -1
    # seven crops over a table of four images, of which only the first is usable: crop 0 and crop 6 are well formed
    order = [0, 1, 0, 0, 0, 0, 1]
    x7, m7, _, _, _ = inp.person_inputs_batch([im], [[centers[i] for i in order]], [[scales[i] for i in order]], [[boxes[i] for i in order]], (192, 256))
    crops_h = x7._i2r_keep[0][:7 * 80].cpu()
    crops_h.numpy().view(inp._CROP_DT)["image"][:] = [0, 7, -1, 1, 2, 3, 0]   # past the table, negative, null img, ih = 0, iw = 0
    images_h = torch.zeros(4 * 24, dtype=torch.uint8)
    iv = images_h.numpy().view(inp._IMG_DT)
    iv[0] = (im.data_ptr(), 120, 160, 480, 0)
    iv[1] = (0, 120, 160, 480, 0)
    iv[2] = (im.data_ptr(), 0, 160, 480, 0)
    iv[3] = (im.data_ptr(), 120, 0, 480, 0)
    crops_d, images_d = crops_h.cuda(), images_h.cuda()
    x = torch.full_like(x7, 5.0)
    m = torch.full_like(m7, 5.0)
    cabi.check(cabi.lib().i2r_person_inputs_cv2(images_d.data_ptr(), 4, crops_d.data_ptr(), 7, 0, mean_c, istd_c, x.data_ptr(), m.data_ptr(), 256, 192, st),
               "i2r_person_inputs_cv2")
    torch.cuda.synchronize()
    assert torch.equal(x[0], x_ref[0]) and torch.equal(m[0], m_ref[0]) and torch.equal(x[6], x_ref[1]) and torch.equal(m[6], m_ref[1])
    assert torch.equal(x[0], x7[0]) and torch.equal(x[6], x7[6])
    for k in range(1, 6):
        assert (x[k] == 0).all() and (m[k] == 0).all(), k


def test_image_to_heatmaps_chain():
    """image bytes -> device crops / masks -> collate -> model: the crops of one image, collated with a second image's, give the same
    heat maps as running that image alone (and the forward accepts what the input side produces)."""
    cfg, sd, _, _, _, _ = setup("w48_l1")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    a = inp.person_inputs(*_scene(1, 240, 320, 2), cfg.MODEL.IMAGE_SIZE)
    b = inp.person_inputs(*_scene(2, 200, 300, 1), cfg.MODEL.IMAGE_SIZE)
    x, m, length = inp.collate([a, b])
    assert length == [2, 1] and x.shape == (3, 3, 256, 192)
    y = net(x, m, length)
    ya = net(a[0], a[1], [2])
    assert torch.isfinite(y).all() and (y[:2] - ya).abs().max().item() < 1e-4


# ---- the scenes of tests/_input_cases.py: float64 geometry, padded rows, the batch path ----
def _dev_norm():
    mean_t = torch.tensor(inp.IMAGENET_MEAN, dtype=torch.float32, device="cuda")
    istd_t = torch.tensor([1.0 / s for s in inp.IMAGENET_STD], dtype=torch.float32, device="cuda")
    return mean_t, istd_t


def _raw_crops(img_t, ih, iw, row_bytes, swap_rb, inv, H, W):
    """i2r_crop_affine_cv2 (inv float64 [n, 6]) or i2r_crop_affine (inv float32 [n, 6]) on a device image of any row pitch"""
    inv = np.ascontiguousarray(inv)
    assert inv.dtype in (np.float64, np.float32) and inv.shape[1] == 6 and img_t.is_cuda and img_t.dtype == torch.uint8
    fn = cabi.lib().i2r_crop_affine_cv2 if inv.dtype == np.float64 else cabi.lib().i2r_crop_affine
    inv_t = torch.from_numpy(inv).cuda()
    mean_t, istd_t = _dev_norm()
    x = torch.empty(inv.shape[0], 3, H, W, dtype=torch.float32, device="cuda")
    cabi.check(fn(img_t.data_ptr(), ih, iw, row_bytes, int(swap_rb), inv_t.data_ptr(), mean_t.data_ptr(), istd_t.data_ptr(), x.data_ptr(),
                  inv.shape[0], H, W, torch.cuda.current_stream().cuda_stream), "crop")
    torch.cuda.synchronize()
    return x


def _raw_masks(boxes, ih, iw, H, W, fixed_point):
    fn = cabi.lib().i2r_box_mask_cv2 if fixed_point else cabi.lib().i2r_box_mask
    bx = torch.tensor(boxes, dtype=torch.int32, device="cuda")
    m = torch.empty(len(boxes), 1, H, W, dtype=torch.float32, device="cuda")
    cabi.check(fn(bx.data_ptr(), ih, iw, m.data_ptr(), len(boxes), H, W, torch.cuda.current_stream().cuda_stream), "mask")
    torch.cuda.synchronize()
    return m


def _run(c, fixed_point):
    """the case through input.person_inputs, or -- rotated and directly given maps -- through the raw C ABI -> numpy (x, mask)"""
    W, H = c.size
    if c.raw:
        img_t = torch.from_numpy(np.array(c.img)).cuda()
        x = _raw_crops(img_t, c.ih, c.iw, 3 * c.iw, c.swap_rb, c.inv() if fixed_point else c.inv32(), H, W)
        m = _raw_masks(c.boxes_int(), c.ih, c.iw, H, W, fixed_point)
    else:
        x, m = inp.person_inputs(np.array(c.img), list(c.centers), list(c.scales), [tuple(b) for b in c.boxes], c.size, color_rgb=c.swap_rb,
                                 fixed_point=fixed_point)
        torch.cuda.synchronize()
    assert x.shape == (c.n, 3, H, W) and m.shape == (c.n, 1, H, W)
    return x.cpu().numpy(), m.cpu().numpy()


@pytest.mark.parametrize("name", ic.NAMES)
def test_fixed_point_kernels_over_the_case_list(name):
    """i2r_crop_affine_cv2 / i2r_box_mask_cv2: the 8-bit level of every pixel, recovered as rint((x std + mean) 255), equals the
    restatement's as an integer, masks bit for bit; and, independently of the restatement, the levels lie within the float64 bounds of
    the geometry (ic.crop_bound, ic.MASK_BOUND: derivations there)."""
    c = ic.BY_NAME[name]
    x, m = _run(c, True)
    ref_lv, ref_mk = ic.restated(name)
    lf = ic.levels_of(x)
    lv = np.rint(lf)
    # a level passes through four fp32 operations on the way out and two float32 constants on the way back: 13 * 2^-24 * 255 (ic.FP32_LEVELS)
    assert np.abs(lf - lv).max() <= ic.FP32_LEVELS
    assert np.array_equal(lv.astype(np.int64), ref_lv.astype(np.int64))
    mean32, istd32 = np.asarray(inp.IMAGENET_MEAN, np.float32), np.asarray([1.0 / s for s in inp.IMAGENET_STD], np.float32)
    ref_x = (ref_lv.astype(np.float32) * np.float32(1.0 / 255.0) - mean32[None, :, None, None]) * istd32[None, :, None, None]
    assert np.abs(x - ref_x).max() < 1e-5                     # (the float normalisation may differ in the last bit)
    assert np.array_equal(m[:, 0], ref_mk.astype(np.float32) * np.float32(1.0 / 255.0))
    value, g, mask64 = ic.modelled(name)
    dev = np.abs(lv - value) / ic.crop_bound(g, 0.0)
    mdev = np.abs(np.rint(m[:, 0].astype(np.float64) * 255.0) - mask64)
    print("%s: crop worst %.3f of its bound, mask worst %.3f levels" % (name, dev.max(), mdev.max()))
    assert (np.abs(lv - value) <= ic.crop_bound(g, 0.0)).all()
    assert mdev.max() <= ic.MASK_BOUND
    for k, who in enumerate(c.who):
        if who in ic.OUTSIDE:     # every pixel (0 - mean) / std exactly, the mask all 0
            assert np.array_equal(x[k], np.broadcast_to(ic.zero_level()[:, None, None], x[k].shape)) and not m[k].any()


@pytest.mark.parametrize("name", ic.NAMES)
def test_fp32_kernels_over_the_case_list(name):
    """i2r_crop_affine / i2r_box_mask against the float64 models evaluated at the float32-rounded inverse map: the crop within
    coordinate error * (Gx + Gy) plus 16 fp32 round-offs of 255 (ic.fp32_coord_err, ic.FP32_LEVELS: derived there, not tuned), the mask
    -- no 8-bit rounding, no odd-size shift -- within 1e-6"""
    c = ic.BY_NAME[name]
    x, m = _run(c, False)
    value, g, mask64 = ic.modelled(name, True)
    tol = ic.fp32_coord_err(c.inv32(), c.size[1], c.size[0])[:, None, None, None] * g + ic.FP32_LEVELS
    err = np.abs(ic.levels_of(x) - value)
    merr = np.abs(m[:, 0].astype(np.float64) - mask64 / 255.0)
    print("%s: crop worst %.3f of its tolerance (worst tolerance %.2e levels), mask worst %.2e" % (name, (err / tol).max(), tol.max(), merr.max()))
    assert (err <= tol).all()
    assert merr.max() < 1e-6


def _padded(img, pad=5):
    """[ih, iw + pad, 3] device tensor whose pad columns hold 255 (a read past column iw - 1 shows), and its row pitch in bytes"""
    ih, iw = img.shape[:2]
    buf = np.full((ih, iw + pad, 3), 255, np.uint8)
    buf[:, :iw] = img
    return torch.from_numpy(buf).cuda(), 3 * (iw + pad)


@pytest.mark.parametrize("name", ["rot0-97x131-48x64", "rot+30-97x131-17x23", "noise-40x30-17x23"])
def test_padded_rows_are_bit_identical_to_contiguous_ones(name):
    """row_bytes > 3 iw through i2r_crop_affine_cv2, i2r_crop_affine and the image table of i2r_person_inputs_cv2"""
    c = ic.BY_NAME[name]
    W, H = c.size
    flat = torch.from_numpy(np.array(c.img)).cuda()
    wide, pitch = _padded(c.img)
    for inv in (c.inv(), c.inv32()):
        a = _raw_crops(flat, c.ih, c.iw, 3 * c.iw, c.swap_rb, inv, H, W)
        b = _raw_crops(wide, c.ih, c.iw, pitch, c.swap_rb, inv, H, W)
        assert torch.equal(a, b)
    x_ref, m_ref, _, _, _ = inp.person_inputs_batch([flat], [list(c.centers)], [list(c.scales)], [[tuple(b) for b in c.boxes]], c.size, color_rgb=c.swap_rb)
    tab_h = x_ref._i2r_keep[0].cpu()           # [crop table (n x 80 bytes) | image table | ...]
    entry = tab_h.numpy()[c.n * 80:c.n * 80 + 24].view(inp._IMG_DT)
    assert entry["img"][0] == flat.data_ptr() and entry["row_bytes"][0] == 3 * c.iw
    entry["img"][0], entry["row_bytes"][0] = wide.data_ptr(), pitch
    tab = tab_h.cuda()
    x, m = torch.full_like(x_ref, 5.0), torch.full_like(m_ref, 5.0)
    mean_c = (C.c_float * 3)(*inp.IMAGENET_MEAN)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in inp.IMAGENET_STD])
    cabi.check(cabi.lib().i2r_person_inputs_cv2(tab.data_ptr() + c.n * 80, 1, tab.data_ptr(), c.n, int(c.swap_rb), mean_c, istd_c, x.data_ptr(),
                                                m.data_ptr(), H, W, torch.cuda.current_stream().cuda_stream), "i2r_person_inputs_cv2")
    torch.cuda.synchronize()
    assert torch.equal(x, x_ref) and torch.equal(m, m_ref)
    if not c.raw:   # (and the table path is the per-image path)
        assert np.array_equal(x.cpu().numpy(), _run(c, True)[0])


@pytest.mark.parametrize("size", ic.SIZES)
def test_batch_path_over_the_case_images(size):
    """one person_inputs_batch call over every case image but the 1080 x 1920 one (sizes from 1 x 1 to 7 x 200, eleven persons each):
    bit-identical to person_inputs per image + collate; the centres / scales it returns are the ones it was given"""
    cs = [c for c in ic.CASES if c.family in ("rot0", "noise") and c.size == size]
    assert len(cs) == len(ic.IMAGES) + 2
    rgb = size == ic.SIZES[0]
    args = [(list(c.centers), list(c.scales), [tuple(b) for b in c.boxes]) for c in cs]
    per_image = [inp.person_inputs(np.array(c.img), *a, size, color_rgb=rgb) for c, a in zip(cs, args)]
    x_ref, m_ref, len_ref = inp.collate(per_image)
    imgs = [torch.from_numpy(np.array(c.img)).cuda() for c in cs]
    x, m, length, cen, scl = inp.person_inputs_batch(imgs, [a[0] for a in args], [a[1] for a in args], [a[2] for a in args], size, color_rgb=rgb)
    torch.cuda.synchronize()
    assert length == len_ref == [c.n for c in cs]
    assert torch.equal(x, x_ref) and torch.equal(m, m_ref)
    assert np.array_equal(cen.cpu().numpy(), np.concatenate([c.centers for c in cs])) and np.array_equal(scl.cpu().numpy(), np.concatenate([c.scales for c in cs]))
