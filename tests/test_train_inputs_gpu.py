"""-m gpu: i2r_train_inputs_cv2 / input.train_inputs_batch (training samples on the device: augmented crops, rotated box masks, joints)
against the materialised CPU composition of tests/_train_input_ref.py (bit for bit), against the reference-written fixture, against
input.person_inputs_batch at the identity augmentation, under a host-side mirror, against float64 geometry that shares nothing with the
fixed-point restatement, on malformed tables and arguments, and end to end into the head re-fit."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

import _head_fit_ref as hfref
import _input_cases as cases
import _train_input_ref as tref
import _val_ref
from _golden import setup
from i2r_amd import cabi, caller, models
from i2r_amd import input as inp
from test_val_metrics_gpu import analytic_loss_bound

pytestmark = pytest.mark.gpu

SIZES = ((48, 64), (17, 23))                                    # (W, H); 17 x 23 = 391 pixels: the last workgroup is partial
IMAGES = ((97, 131), (96, 130), (40, 30), (7, 200), (1, 1))     # (ih, iw); 40 x 30: the mask is magnified
ROTATIONS = (0, 30.0, -17.0, 90.0, 180.0, 80.0)
GUARD, POISON = 1024, -4321.25
MARGIN = 3.0                                                    # source pixels, see test_masks_follow_the_float64_rectangle


def dev():
    return torch.device("cuda", 0)


def person_boxes(ih, iw):
    t = cases.persons(ih, iw)
    return [t[k] for k in ("interior", "right", "bottom", "larger", "outside+")]


def entry_rows(boxes, ih, iw, size, rot, flip, image=0, sf=1.15):
    """table rows for the persons `boxes` (x, y, w, h) of one image under one augmentation -> (rows, trans [n, 2, 3], boxes_int)"""
    rows = np.zeros(len(boxes), dtype=inp._TRAIN_CROP_DT)
    cs = [inp.box_to_center_scale(b, size) for b in boxes]
    trans = np.stack([inp.train_affine_transform(c, s.astype(np.float64) * sf, rot, size) for c, s in cs])
    M, nW, nH = inp.rotate_bound_geometry(ih, iw, rot)
    bi = np.array([[int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])] for b in boxes], dtype=np.int32)
    rows["inv_m"] = inp.cv2_inverse_batch(trans)
    rows["mask_inv_m"] = inp.cv2_inverse(M).reshape(6)
    rows["box"], rows["nw"], rows["nh"], rows["image"], rows["flip"] = bi, nW, nH, image, int(flip)
    return rows, trans, bi


def launch(imgs, rows, size, swap_rb=False, expect=0, **override):
    """the raw C-ABI call on poisoned outputs between canaries.  imgs: list of uint8 numpy [ih, iw, 3] (or prepared image-table rows
    via image_rows=); other keywords replace arguments of the call -> (x [S, 3, H, W], mask [S, 1, H, W]) numpy, or None where expect != 0 (outputs verified untouched)"""
    W, H = size
    S = len(rows)
    keep = [torch.from_numpy(np.array(im, order="C", copy=True)).to(dev()) for im in imgs]   # (a fresh copy: writable, plain strides)
    irows = np.zeros(len(imgs), dtype=inp._IMG_DT)
    for i, t in enumerate(keep):
        irows[i] = (t.data_ptr(), t.shape[0], t.shape[1], t.shape[1] * 3, 0)
    irows = override.pop("image_rows", irows)
    itab = torch.from_numpy(irows.view(np.uint8).copy()).to(dev())
    ctab = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).copy()).to(dev())
    xb = torch.full((S * 3 * H * W + 2 * GUARD,), POISON, dtype=torch.float32, device=dev())
    mb = torch.full((S * H * W + 2 * GUARD,), POISON, dtype=torch.float32, device=dev())
    mean_c = (C.c_float * 3)(*inp.IMAGENET_MEAN)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in inp.IMAGENET_STD])
    a = dict(images=itab.data_ptr(), n_images=len(irows), crops=ctab.data_ptr(), n_crops=S, swap_rb=int(swap_rb), mean=mean_c, inv_std=istd_c,
             x_out=xb.data_ptr() + 4 * GUARD, mask_out=mb.data_ptr() + 4 * GUARD, oh=H, ow=W)
    a.update(override)
    rc = cabi.lib().i2r_train_inputs_cv2(a["images"], a["n_images"], a["crops"], a["n_crops"], a["swap_rb"], a["mean"], a["inv_std"], a["x_out"],
                                         a["mask_out"], a["oh"], a["ow"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    xh, mh = xb.cpu().numpy(), mb.cpu().numpy()
    for h in (xh, mh):
        assert (h[:GUARD] == POISON).all() and (h[-GUARD:] == POISON).all(), "canary overwritten"
    if expect != 0:
        assert (xh == POISON).all() and (mh == POISON).all(), "an argument error launched something"
        return None
    return xh[GUARD:-GUARD].reshape(S, 3, H, W), mh[GUARD:-GUARD].reshape(S, 1, H, W)


def assert_same_levels(x, m, crops_u8, masks_u8, what=""):
    """masks bit for bit; crops at the same 8-bit level (the fp32 normalisation may differ in its last bit: the bar of test_input_gpu.py)"""
    want_m = masks_u8.astype(np.float32) * np.float32(1.0 / 255.0)
    assert np.array_equal(m[:, 0], want_m), "%s: %d mask pixels differ" % (what, int((m[:, 0] != want_m).sum()))
    d = np.abs(x - tref.normalised(crops_u8)).max()
    assert d < 1e-5, "%s: crop differs by %.3g" % (what, d)


# ---- the fixture: the reference's own __getitem__ ----------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(tref.fixture().samples)))
def test_fixture_samples_through_train_inputs_batch(i):
    f = tref.fixture()
    s = f.samples[i]
    st = f.sets[s.set]
    _, g, _ = tref.replay(i)
    im = torch.from_numpy(np.array(st.image)).to(dev())
    r = inp.train_inputs_batch([im], None, None, st.image_size, st.heatmap_size, geometry=[g])
    torch.cuda.synchronize()
    assert r.length == [3] and r.rotation == [s.rot] and r.flip == [s.flip]
    assert_same_levels(r.x.cpu().numpy(), r.pos_mask.cpu().numpy(), s.crops, s.masks, "sample %d" % i)
    assert r.joints_hm.dtype == torch.float64 and r.joints_vis.dtype == torch.float32
    assert np.array_equal(r.joints_hm.cpu().numpy(), g.joints_hm[:, :, :2]) and np.array_equal(r.joints.cpu().numpy(), g.joints[:, :, :2])
    assert np.array_equal(r.joints_vis.cpu().numpy(), s.joints_vis[:, :, 0].astype(np.float32))
    assert np.array_equal(r.center.cpu().numpy(), g.center.astype(np.float32)) and np.array_equal(r.scale.cpu().numpy(), g.scale.astype(np.float32))


# ---- constructed scenes: every image size x output size, all rotations and both flips in one launch ---------------------------------

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shape", IMAGES)
def test_constructed_scenes_equal_the_materialised_composition(shape, size):
    ih, iw = shape
    img = cases.image("noise" if shape == (40, 30) else "smooth", ih, iw)
    swap = (ih + size[0]) % 2 == 1
    boxes = person_boxes(ih, iw)
    rows, want_c, want_m = [], [], []
    for rot in ROTATIONS:
        for flip in (False, True):
            r, trans, bi = entry_rows(boxes, ih, iw, size, rot, flip)
            c, m = tref.materialised(img, trans, bi, rot, flip, size, swap_rb=swap)
            rows.append(r), want_c.append(c), want_m.append(m)
    x, m = launch([img], np.concatenate(rows), size, swap_rb=swap)
    want_c, want_m = np.concatenate(want_c), np.concatenate(want_m)
    assert_same_levels(x, m, want_c, want_m, "%dx%d -> %dx%d" % (ih, iw, size[0], size[1]))
    n = len(boxes)
    outside = m[n - 1::n]                                               # the person far outside the image, under every augmentation
    assert (outside == 0).all() and np.abs(x[n - 1::n] - cases.zero_level()[None, :, None, None]).max() < 1e-5
    if min(ih, iw) >= 30:
        assert (m == 1.0).any() and ((m > 0) & (m < 1)).any()


def test_one_batch_of_three_images_of_different_sizes():
    """3 / 1 / 2 persons, each image its own draw, through input.train_inputs_batch with the draws (the coins from a seeded generator)"""
    f = tref.fixture()
    st = f.sets[1]                                                       # 14 joints
    shapes, counts = ((97, 131), (40, 30), (96, 130)), (3, 1, 2)
    draws = [(30.0, 1.2, True, True), (0, 0.8, False, False), (-17.0, 1.0, True, False)]
    imgs, annos = [], []
    for k, ((ih, iw), n) in enumerate(zip(shapes, counts)):
        imgs.append(cases.image("smooth", ih, iw))
        sx, sy = iw / 130.0, ih / 96.0
        al = []
        for a in st.annos[:n]:
            j = np.array(a["joints_3d"])
            j[:, 0] *= sx
            j[:, 1] *= sy
            box = np.array(a["box"]) * [sx, sy, sx, sy]
            c, s = inp.box_to_center_scale(box, (48, 64))
            al.append(dict(joints_3d=j, joints_3d_vis=a["joints_3d_vis"], center=c, scale=s, box=box))
        annos.append(al)
    dimgs = [torch.from_numpy(np.array(im)).to(dev()) for im in imgs]
    rs = np.random.RandomState(0)
    r = inp.train_inputs_batch(dimgs, annos, draws, (48, 64), (12, 16), dataset="crowdpose", color_rgb=True, np_random=rs)
    torch.cuda.synchronize()
    assert r.length == [3, 1, 2] and r.x.shape == (6, 3, 64, 48) and r.pos_mask.shape == (6, 1, 64, 48)
    assert r.rotation == [30.0, 0, -17.0] and r.flip == [True, False, False]
    x, m = r.x.cpu().numpy(), r.pos_mask.cpu().numpy()
    o = 0
    for k in range(3):
        g = r.geometry[k]
        c, mk = tref.materialised(imgs[k], g.trans, g.box, g.rotation, g.flip, (48, 64), swap_rb=True)
        assert_same_levels(x[o:o + counts[k]], m[o:o + counts[k]], c, mk, "image %d" % k)
        assert np.array_equal(r.joints_hm[o:o + counts[k]].cpu().numpy(), g.joints_hm[:, :, :2])
        o += counts[k]
    assert inp.HALF_BODY_UPPER in r.geometry[0].half_body or inp.HALF_BODY_LOWER in r.geometry[0].half_body
    assert r.x._i2r_keep is r._i2r_keep and r._i2r_keep[1][0] is dimgs[0]


# ---- against the validation kernel, and under a host-side mirror ---------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shape", IMAGES)
def test_identity_augmentation_is_bit_identical_to_person_inputs_batch(shape, size):
    """r = 0, no flip, the maps person_inputs_batch itself builds: crop AND mask equal the validation kernel's bit for bit (the general
    mask path at rot 0 against mask_pixel_cv2's odd-size shift)"""
    ih, iw = shape
    img = cases.image("smooth", ih, iw)
    boxes = list(cases.persons(ih, iw).values())
    cs = [inp.box_to_center_scale(b, size) for b in boxes]
    cen, scl = np.stack([c for c, _ in cs]), np.stack([s for _, s in cs])
    im = torch.from_numpy(np.array(img)).to(dev())
    x_ref, m_ref, _, _, _ = inp.person_inputs_batch([im], [cen], [scl], [boxes], size, color_rgb=True)
    rows, _, _ = entry_rows(boxes, ih, iw, size, 0, False)
    rows["inv_m"] = inp.cv2_inverse_batch(inp.affine_transforms(cen, scl, size))
    assert (rows["nw"] == iw).all() and (rows["nh"] == ih).all()
    x, m = launch([img], rows, size, swap_rb=True)
    assert np.array_equal(x, x_ref.cpu().numpy()) and np.array_equal(m, m_ref.cpu().numpy())


@pytest.mark.parametrize("shape", IMAGES)
def test_flip_equals_no_flip_on_a_mirrored_image_and_boxes(shape):
    ih, iw = shape
    size = SIZES[(ih + iw) % 2]
    img = cases.image("noise", ih, iw)
    boxes = person_boxes(ih, iw)
    on, off = [], []
    for rot in ROTATIONS:
        a, _, bi = entry_rows(boxes, ih, iw, size, rot, True)
        b = a.copy()
        b["flip"] = 0
        b["box"] = np.stack([iw - 1 - bi[:, 2], bi[:, 1], iw - 1 - bi[:, 0], bi[:, 3]], 1)
        on.append(a), off.append(b)
    x1, m1 = launch([img], np.concatenate(on), size)
    x0, m0 = launch([np.ascontiguousarray(img[:, ::-1])], np.concatenate(off), size)
    assert np.array_equal(x1, x0) and np.array_equal(m1, m0)
    if iw > 1:
        xn, _ = launch([img], np.concatenate(off), size)
        assert not np.array_equal(xn, x1)


# ---- geometry against float64, independent of the fixed-point restatement ----------------------------------------------------------

GEO_IMAGES = ((97, 131), (96, 130), (40, 30))


def geo_box(ih, iw):
    return (0.15 * iw, 0.15 * ih, 0.7 * iw, 0.7 * ih)


@functools.lru_cache(maxsize=None)
def geo_run(shape, size):
    ih, iw = shape
    img = cases.image("smooth", ih, iw)
    rows = np.concatenate([entry_rows([geo_box(ih, iw)], ih, iw, size, rot, flip, sf=1.0)[0] for rot in ROTATIONS for flip in (False, True)])
    x, m = launch([img], rows, size)
    return img, rows, x, m


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shape", GEO_IMAGES)
def test_crops_follow_the_float64_interpolant(shape, size):
    """bilinear interpolation of the UNFLIPPED image at the exact source coordinate, the mirror composed into the inverse map
    (sx -> iw - 1 - sx), within crop_bound"""
    img, rows, x, _ = geo_run(shape, size)
    W, H = size
    iw = shape[1]
    lv = cases.levels_of(x)
    worst = 0.0
    for p, row in enumerate(rows):
        m = row["inv_m"].copy()
        if row["flip"]:
            m[:3] = [-m[0], -m[1], iw - 1 - m[2]]
        val, gx, gy = cases.crop_f64(img, m, H, W)
        ratio = np.abs(lv[p].transpose(1, 2, 0) - val) / cases.crop_bound(gx, gy)
        worst = max(worst, float(ratio.max()))
    print("%s -> %s: max |level - model| / bound %.3f" % (shape, size, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("shape", GEO_IMAGES)
def test_masks_follow_the_float64_rectangle(shape, size):
    """Every output pixel is classified by where its exact float64 source point lies: output centre -> canvas coordinate
    ((x + 0.5) nW / W - 0.5) -> mask_inv_m -> the image, mirrored back where flipped.  At least MARGIN = 3 source pixels inside the
    clipped rectangle the mask must be exactly 1, at least 3 outside exactly 0: the two resize taps lie within 1 px per axis of the canvas
    coordinate, the bilinear taps of the warp within another 1 px per axis (the rotation is an isometry: canvas px = source px), the
    fixed-point coordinate adds 1/64 + 1/1024: 2 sqrt(2) + 0.03 < 3."""
    ih, iw = shape
    _, rows, _, m = geo_run(shape, size)
    W, H = size
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for p, row in enumerate(rows):
        u = (xs + 0.5) * (float(row["nw"]) / W) - 0.5
        v = (ys + 0.5) * (float(row["nh"]) / H) - 0.5
        k = row["mask_inv_m"]
        sx, sy = k[0] * u + k[1] * v + k[2], k[3] * u + k[4] * v + k[5]
        if row["flip"]:
            sx = iw - 1 - sx
        x0, y0, x1, y1 = max(row["box"][0], 0), max(row["box"][1], 0), min(row["box"][2], iw - 1), min(row["box"][3], ih - 1)
        inside = np.minimum(np.minimum(sx - x0, x1 - sx), np.minimum(sy - y0, y1 - sy))          # > 0 inside, the distance to the nearest edge
        dx, dy = np.maximum(np.maximum(x0 - sx, sx - x1), 0), np.maximum(np.maximum(y0 - sy, sy - y1), 0)
        outside = np.hypot(dx, dy)
        is_in, is_out = inside >= MARGIN, outside >= MARGIN
        assert is_in.sum() >= 50 and is_out.sum() >= 50, (p, int(is_in.sum()), int(is_out.sum()))
        assert (m[p, 0][is_in] == 1.0).all() and (m[p, 0][is_out] == 0.0).all(), (p, row["flip"])


# ---- robustness -----------------------------------------------------------------------------------------------------------------------

def test_invalid_table_entries_write_zeros_and_leave_their_neighbours_alone():
    ih, iw, size = 96, 130, SIZES[1]
    img = cases.image("smooth", ih, iw)
    boxes = [cases.persons(ih, iw)["interior"]] * 8
    rows, _, _ = entry_rows(boxes, ih, iw, size, 30.0, True)
    good = launch([img], rows[:1], size)[0]
    bad = rows.copy()
    bad["image"][1], bad["image"][2] = -1, 2            # outside the table of two images, both ways
    bad["image"][3] = 1                                 # image 1 is made empty below: null pointer
    bad["nw"][4], bad["nh"][5] = 0, -3                  # empty canvas
    bad["image"][6] = 2 ** 31 - 1
    keep = torch.from_numpy(np.array(img)).to(dev())
    irows = np.zeros(2, dtype=inp._IMG_DT)
    irows[0] = (keep.data_ptr(), ih, iw, iw * 3, 0)
    irows[1] = (0, ih, iw, iw * 3, 0)
    x, m = launch([], bad, size, image_rows=irows)
    for p in (1, 2, 3, 4, 5, 6):
        assert (x[p] == 0).all() and (m[p] == 0).all(), p
    for p in (0, 7):
        assert np.array_equal(x[p], good[0]) and m[p].max() == 1.0
    for col in ("ih", "iw"):                            # an image entry without rows or columns
        ir = irows.copy()
        ir[col][0] = 0
        x, m = launch([], bad, size, image_rows=ir)
        assert (x == 0).all() and (m == 0).all()


def test_argument_errors_are_codes_not_launches():
    ih, iw, size = 40, 30, SIZES[1]
    img = cases.image("smooth", ih, iw)
    rows, _, _ = entry_rows(person_boxes(ih, iw), ih, iw, size, 30.0, False)
    assert launch([img], rows, size) is not None
    for kw in (dict(images=None), dict(crops=None), dict(mean=None), dict(inv_std=None), dict(x_out=None), dict(mask_out=None),
               dict(n_images=0), dict(n_images=-1), dict(n_crops=0), dict(n_crops=-2), dict(oh=0), dict(ow=0), dict(oh=-5),
               dict(n_crops=2 ** 31 - 1, oh=2 ** 15, ow=2 ** 15)):
        assert launch([img], rows, size, expect=-1, **kw) is None, kw
        assert b"i2r_train_inputs_cv2" in cabi.lib().i2r_last_error()


# ---- end to end: decoded frames -> augmented batch -> frozen features -> the head's loss and gradient ---------------------------------

def test_end_to_end_into_the_head_refit():
    cfg, sd, _, _, length, _ = setup("tph_l21")
    net = models.interformer.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    J = cfg.MODEL.NUM_JOINTS
    size, hsize = tuple(cfg.MODEL.IMAGE_SIZE), tuple(cfg.MODEL.HEATMAP_SIZE)
    assert J == 14 and size == (192, 256)
    rng = np.random.RandomState(7)
    shapes = ((240, 320), (333, 517), (121, 90))[:len(length)]
    imgs, annos, draws = [], [], []
    py = random.Random(7)
    for (ih, iw), n in zip(shapes, length):
        imgs.append(torch.from_numpy(cases.smooth_image(ih, iw, ih)).to(dev()))
        al = []
        for p in range(n):
            w, h = rng.uniform(0.3, 0.6) * iw, rng.uniform(0.5, 0.9) * ih
            box = np.array([rng.uniform(0, iw - w), rng.uniform(0, ih - h), w, h])
            joints = np.zeros((J, 3))
            joints[:, 0], joints[:, 1] = rng.uniform(box[0], box[0] + w, J), rng.uniform(box[1], box[1] + h, J)
            vis = np.zeros((J, 3))
            vis[:, :2] = (rng.rand(J) < 0.8)[:, None]
            joints[vis[:, 0] == 0] = 0
            c, s = inp.box_to_center_scale(box, size)
            al.append(dict(joints_3d=joints, joints_3d_vis=vis, center=c, scale=s, box=box))
        annos.append(al)
        draws.append(inp.draw_augmentation(0.35, 45, True, 0.3, np_random=rng, py_random=py))
    t = inp.train_inputs_batch(imgs, annos, draws, size, hsize, dataset="crowdpose", color_rgb=cfg.DATASET.COLOR_RGB, np_random=rng)
    assert t.length == list(length)
    hi = net.head_input(t.x, t.pos_mask, t.length)
    fit = caller.HeadFit.from_model(net)
    g = fit.grad(hi.feat, joints_hm=t.joints_hm, joints_vis=t.joints_vis)
    vm = caller.val_metrics_cfg(cfg, hi.heatmaps, joints_hm=t.joints_hm, joints_vis=t.joints_vis)
    loss = fit.step(hi.feat, joints_hm=t.joints_hm, joints_vis=t.joints_vis)
    torch.cuda.synchronize()
    mu, vis = t.joints_hm.cpu().numpy(), t.joints_vis.cpu().numpy()
    jw = caller.JOINTS_WEIGHT["crowdpose"] if cfg.LOSS.USE_DIFFERENT_JOINTS_WEIGHT else None
    w, h = hsize
    target, tw = _val_ref.joint_targets(mu, vis, h, w, cfg.MODEL.SIGMA, jw)
    _, tw_plain = _val_ref.joint_targets(mu, vis, h, w, cfg.MODEL.SIGMA, None)
    wt, b = sd["final_layer.weight"].reshape(J, -1).numpy(), sd["final_layer.bias"].numpy()
    use_w = bool(cfg.LOSS.USE_TARGET_WEIGHT)
    feat = hi.feat.cpu().numpy()
    pad = np.zeros((J, feat.shape[3]), np.float32)
    pad[:, :wt.shape[1]] = wt
    r64 = hfref.head_grad64(feat, pad[:, :(wt.shape[1] + 15) // 16 * 16], b, target, tw, use_w, drawn=tw_plain > 0.5)
    vm_bound = analytic_loss_bound(hi.heatmaps.cpu().numpy(), target, tw, use_w)
    diff = abs(g.loss.item() - vm.loss.item())
    print("head_grad loss %.17g, val_metrics %.17g, float64 %.17g, |diff| %.3g, bound %.3g + %.3g"
          % (g.loss.item(), vm.loss.item(), r64.loss, diff, r64.b_loss, vm_bound))
    assert (tw > 0).sum() >= J and np.isfinite(g.loss.item()) and g.loss.item() > 0
    assert diff <= r64.b_loss + vm_bound
    assert abs(g.loss.item() - r64.loss) <= r64.b_loss and loss.item() == g.loss.item()
