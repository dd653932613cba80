"""Input side of the path on the device: what JointsDataset.__getitem__ + collater do on the CPU with
cv2 for every person of an image (reference lib/dataset/JointsDataset.py:207-356, lib/dataset/collater.py:14-26,175-183):

    crops, masks = person_inputs(image_u8, centers, scales, boxes, cfg)     # per image: [n,3,H,W], [n,1,H,W] on the GPU
    x, pos_mask, length = collate([(crops0, masks0), (crops1, masks1), ...])  # -> model(x, pos_mask, length)

The affine matrices are built on the host in float64 exactly as lib/utils/transforms.py:61-96 does (cv2.getAffineTransform is a
3-point solve); interpolation runs in csrc/i2r_input.hip -- by default in cv2's own fixed-point arithmetic (restated from OpenCV's
published algorithm: 1/32-pixel coordinates, 15-bit weights, 8-bit results, the half-pixel shift rotate_bound applies to masks of
odd-sized images), optionally in plain fp32.  cv2 itself is absent here, so this step is NOT pinned against a cv2 output; its
geometry is pinned to float64 models of the crop and the mask (tests/_input_cases.py).

The TRAINING half of __getitem__ (JointsDataset.py:233-334: random rotation and scale, flip with left / right swap, half-body crop, the
rotated pos_mask) is here too: draw_augmentation and train_geometry restate the host arithmetic in the reference's order and number
formats, train_inputs_batch builds the batch on the device (i2r_train_inputs_cv2) with the joints in heat-map coordinates beside it."""
import ctypes as C
import random

import numpy as np
import torch

from . import cabi

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # tools/test.py:126-128
IMAGENET_STD = (0.229, 0.224, 0.225)


def _third_point(a, b):
    d = a - b
    return b + np.array([-d[1], d[0]], dtype=np.float64)


def get_affine_transform(center, scale, rot, output_size, shift=(0.0, 0.0), inv=0):
    """lib/utils/transforms.py:61-96 -> 2x3 float64.  cv2.getAffineTransform(src, dst) maps three point pairs; the pairs are rounded
    to float32 first like the reference does (np.float32(src))."""
    scale = np.asarray(scale, dtype=np.float64).reshape(-1)
    if scale.size == 1:
        scale = np.array([scale[0], scale[0]])
    center = np.asarray(center, dtype=np.float64)
    shift = np.asarray(shift, dtype=np.float64)
    scale_tmp = scale * 200.0
    src_w = scale_tmp[0]
    dst_w, dst_h = float(output_size[0]), float(output_size[1])
    rot_rad = np.pi * rot / 180.0
    sn, cs = np.sin(rot_rad), np.cos(rot_rad)
    p = np.array([0.0, (src_w - 1) * -0.5])
    src_dir = np.array([p[0] * cs - p[1] * sn, p[0] * sn + p[1] * cs])
    dst_dir = np.array([0.0, (dst_w - 1) * -0.5])
    src = np.zeros((3, 2), dtype=np.float32)
    dst = np.zeros((3, 2), dtype=np.float32)
    src[0] = center + scale_tmp * shift
    src[1] = center + src_dir + scale_tmp * shift
    dst[0] = [(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]
    dst[1] = np.array([(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]) + dst_dir
    src[2] = _third_point(src[0].astype(np.float64), src[1].astype(np.float64))
    dst[2] = _third_point(dst[0].astype(np.float64), dst[1].astype(np.float64))
    a, b = (dst, src) if inv else (src, dst)
    A = np.concatenate([a.astype(np.float64), np.ones((3, 1))], axis=1)   # [x y 1] T^T = [x' y']
    return np.linalg.solve(A, b.astype(np.float64)).T


def invert_affine(t):
    """cv2.invertAffineTransform: the dst -> src map warpAffine iterates over."""
    t = np.asarray(t, dtype=np.float64)
    A = np.linalg.inv(t[:, :2])
    return np.concatenate([A, -A @ t[:, 2:]], axis=1)


def box_to_center_scale(box, image_size, pixel_std=200.0):
    """_box2cs / _xywh2cs of the dataset classes (lib/dataset/crowdpose.py:239-258, coco.py, ochuman.py): box (x, y, w, h) -> centre
    of the box and the aspect-corrected scale (in units of pixel_std = 200 px, enlarged by 1.25), both float32 like the reference."""
    x, y, w, h = [float(v) for v in box[:4]]
    aspect = float(image_size[0]) / float(image_size[1])
    center = np.array([x + (w - 1) * 0.5, y + (h - 1) * 0.5], dtype=np.float32)
    if w > aspect * h:
        h = w * 1.0 / aspect
    elif w < aspect * h:
        w = h * aspect
    scale = np.array([w * 1.0 / pixel_std, h * 1.0 / pixel_std], dtype=np.float32)
    if center[0] != -1:
        scale = scale * 1.25
    return center, scale


def cv2_inverse(t):
    """the dst -> src matrix cv2.warpAffine derives from a forward 2x3 map (imgwarp.cpp: closed form in double precision)"""
    t = np.asarray(t, dtype=np.float64)
    D = t[0, 0] * t[1, 1] - t[0, 1] * t[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    m = np.array([[t[1, 1] * D, -t[0, 1] * D, 0.0], [-t[1, 0] * D, t[0, 0] * D, 0.0]])
    m[0, 2] = -m[0, 0] * t[0, 2] - m[0, 1] * t[1, 2]
    m[1, 2] = -m[1, 0] * t[0, 2] - m[1, 1] * t[1, 2]
    return m


def person_inputs(image, centers, scales, boxes, image_size, color_rgb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda:0",
                  fixed_point=True):
    """image: uint8 [ih, iw, 3] (numpy or tensor, channel order as cv2.imread delivers it); centers / scales: per-person (2,) pairs in
    the dataset convention (scale in units of 200 px); boxes: per-person (x, y, w, h); image_size = cfg.MODEL.IMAGE_SIZE = (W, H).
    -> (input [n, 3, H, W], pos_mask [n, 1, H, W]) fp32 on `device`, ready for model(input, pos_mask, [n])."""
    dev = torch.device(device)
    img = torch.as_tensor(image)
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
    img = img.to(dev).contiguous()
    ih, iw = int(img.shape[0]), int(img.shape[1])
    n = len(centers)
    assert n >= 1 and len(scales) == n and len(boxes) == n
    W, H = int(image_size[0]), int(image_size[1])
    trans = [get_affine_transform(centers[i], scales[i], 0, (W, H)) for i in range(n)]
    # cv2.rectangle(mask, (int(x), int(y)), (int(x+w), int(y+h)), 255, -1): inclusive corners (JointsDataset.py:168-169)
    bx = torch.tensor([[int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])] for b in boxes], dtype=torch.int32, device=dev)
    mean_t = torch.tensor(mean, dtype=torch.float32, device=dev)
    istd_t = torch.tensor([1.0 / s for s in std], dtype=torch.float32, device=dev)
    x = torch.empty(n, 3, H, W, dtype=torch.float32, device=dev)
    m = torch.empty(n, 1, H, W, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L = cabi.lib()
    if fixed_point:  # cv2's own fixed-point arithmetic (the default: it is what the reference's data loader computes)
        inv_t = torch.from_numpy(np.stack([cv2_inverse(t) for t in trans]).reshape(n, 6)).to(dev)  # float64
        cabi.check(L.i2r_crop_affine_cv2(img.data_ptr(), ih, iw, iw * 3, int(bool(color_rgb)), inv_t.data_ptr(), mean_t.data_ptr(),
                                         istd_t.data_ptr(), x.data_ptr(), n, H, W, st), "i2r_crop_affine_cv2")
        cabi.check(L.i2r_box_mask_cv2(bx.data_ptr(), ih, iw, m.data_ptr(), n, H, W, st), "i2r_box_mask_cv2")
    else:            # fp32 interpolation of the same geometry (no 8-bit rounding, no half-pixel shift of the mask)
        inv_t = torch.from_numpy(np.stack([invert_affine(t) for t in trans]).reshape(n, 6).astype(np.float32)).to(dev)
        cabi.check(L.i2r_crop_affine(img.data_ptr(), ih, iw, iw * 3, int(bool(color_rgb)), inv_t.data_ptr(), mean_t.data_ptr(),
                                     istd_t.data_ptr(), x.data_ptr(), n, H, W, st), "i2r_crop_affine")
        cabi.check(L.i2r_box_mask(bx.data_ptr(), ih, iw, m.data_ptr(), n, H, W, st), "i2r_box_mask")
    return x, m


def affine_transforms(centers, scales, output_size, rot=0):
    """get_affine_transform(center_i, scale_i, rot_i, output_size) for a whole batch of crops at once -> [S, 2, 3] float64.  Same
    arithmetic as the scalar function (three float32-rounded point pairs, one 3x3 solve each -- numpy solves the stack with the same
    LAPACK routine per matrix), so the results are bit-identical to it (tests/test_host.py).  rot: degrees, one value or one per crop."""
    c = np.asarray(centers, dtype=np.float64).reshape(-1, 2)
    sc = np.asarray(scales, dtype=np.float64).reshape(-1, 2) * 200.0
    S = c.shape[0]
    dst_w, dst_h = float(output_size[0]), float(output_size[1])
    src = np.zeros((S, 3, 2), dtype=np.float32)
    dst = np.zeros((S, 3, 2), dtype=np.float32)
    src[:, 0] = c                                            # (+ scale_tmp * shift with shift = 0)
    rot = np.asarray(rot, dtype=np.float64)
    if rot.ndim == 0 and rot == 0:
        src[:, 1, 0] = c[:, 0] + 0.0
        src[:, 1, 1] = c[:, 1] + (sc[:, 0] - 1) * -0.5       # src_dir = (0, (src_w - 1) * -0.5) at rot = 0
    else:
        rot_rad = np.pi * np.broadcast_to(rot, (S,)) / 180.0
        sn, cs = np.sin(rot_rad), np.cos(rot_rad)
        p0, p1 = np.zeros(S), (sc[:, 0] - 1) * -0.5
        src[:, 1, 0] = c[:, 0] + (p0 * cs - p1 * sn)
        src[:, 1, 1] = c[:, 1] + (p0 * sn + p1 * cs)
    dst[:, 0] = [(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]
    dst[:, 1] = np.array([(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]) + np.array([0.0, (dst_w - 1) * -0.5])

    def third(a, b):  # _third_point on float64 copies of the float32-rounded points
        d = a - b
        return b + np.stack([-d[:, 1], d[:, 0]], axis=1)
    src[:, 2] = third(src[:, 0].astype(np.float64), src[:, 1].astype(np.float64))
    dst[:, 2] = third(dst[:, 0].astype(np.float64), dst[:, 1].astype(np.float64))
    A = np.concatenate([src.astype(np.float64), np.ones((S, 3, 1))], axis=2)
    return np.transpose(np.linalg.solve(A, dst.astype(np.float64)), (0, 2, 1))


def cv2_inverse_batch(t):
    """cv2_inverse over [S, 2, 3] -> [S, 6] (same closed form, element-wise)"""
    t = np.asarray(t, dtype=np.float64)
    D = t[:, 0, 0] * t[:, 1, 1] - t[:, 0, 1] * t[:, 1, 0]
    D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
    m = np.zeros((t.shape[0], 6))
    m[:, 0], m[:, 1] = t[:, 1, 1] * D, -t[:, 0, 1] * D
    m[:, 3], m[:, 4] = -t[:, 1, 0] * D, t[:, 0, 0] * D
    m[:, 2] = -m[:, 0] * t[:, 0, 2] - m[:, 1] * t[:, 1, 2]
    m[:, 5] = -m[:, 3] * t[:, 0, 2] - m[:, 4] * t[:, 1, 2]
    return m


_CROP_DT = np.dtype([("inv_m", "<f8", 6), ("box", "<i4", 4), ("image", "<i4"), ("reserved", "<i4", 3)])      # i2r_crop_ref, 80 bytes
_IMG_DT = np.dtype([("img", "<u8"), ("ih", "<i4"), ("iw", "<i4"), ("row_bytes", "<i4"), ("reserved", "<i4")])  # i2r_image_ref, 24 bytes
assert _CROP_DT.itemsize == 80 and _IMG_DT.itemsize == 24


def person_inputs_batch(images, centers, scales, boxes, image_size, color_rgb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda:0"):
    """The input side of a whole validate() batch in ONE launch (i2r_person_inputs_cv2) and ONE pinned, stream-ordered upload:
    images: list of uint8 [ih_i, iw_i, 3] tensors already on `device` (the decoded frames); centers / scales / boxes: per image, lists
    with one entry per person (as person_inputs takes them).  -> (input [S, 3, H, W], pos_mask [S, 1, H, W], length, center_dev [S, 2],
    scale_dev [S, 2]): the collated tensors collater.__call__ would build (lib/dataset/collater.py:14-26), the persons-per-image list for
    model(input, pos_mask, length), and the crops' centres / scales as device tensors for caller.decode.  cv2's fixed-point arithmetic,
    bit-identical to person_inputs + collate."""
    dev = torch.device(device)
    W, H = int(image_size[0]), int(image_size[1])
    length = [len(c) for c in centers]
    S, n_img = sum(length), len(images)
    assert n_img == len(length) == len(scales) == len(boxes) and S >= 1 and all(n >= 1 for n in length)
    cen = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 2) for c in centers])
    scl = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in scales])
    bxs = np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes])
    # one host buffer: [crop table | image table | centres f32 | scales f32], uploaded with a single non-blocking copy from pinned memory
    off_img = S * 80
    off_c = off_img + (n_img * 24 + 15) // 16 * 16
    off_s = off_c + S * 8
    host = torch.empty(off_s + S * 8, dtype=torch.uint8).pin_memory()
    hb = host.numpy()
    crops = hb[:off_img].view(_CROP_DT)
    crops["inv_m"] = cv2_inverse_batch(affine_transforms(cen, scl, (W, H)))
    # cv2.rectangle(mask, (int(x), int(y)), (int(x+w), int(y+h)), 255, -1): inclusive corners, int() truncates (JointsDataset.py:168-169)
    crops["box"] = np.stack([np.trunc(bxs[:, 0]), np.trunc(bxs[:, 1]), np.trunc(bxs[:, 0] + bxs[:, 2]), np.trunc(bxs[:, 1] + bxs[:, 3])], 1).astype(np.int32)
    crops["image"] = np.repeat(np.arange(n_img, dtype=np.int32), length)
    crops["reserved"] = 0
    imgs = hb[off_img:off_img + n_img * 24].view(_IMG_DT)
    for i, im in enumerate(images):
        assert im.is_cuda and im.device == dev and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous()
        imgs[i] = (im.data_ptr(), im.shape[0], im.shape[1], im.shape[1] * 3, 0)
    hb[off_c:off_s].view(np.float32)[:] = cen.astype(np.float32).reshape(-1)
    hb[off_s:].view(np.float32)[:] = scl.astype(np.float32).reshape(-1)
    tab = host.to(dev, non_blocking=True)
    x = torch.empty(S, 3, H, W, dtype=torch.float32, device=dev)
    m = torch.empty(S, 1, H, W, dtype=torch.float32, device=dev)
    mean_c = (C.c_float * 3)(*mean)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in std])
    st = torch.cuda.current_stream(dev).cuda_stream
    cabi.check(cabi.lib().i2r_person_inputs_cv2(tab.data_ptr() + off_img, n_img, tab.data_ptr(), S, int(bool(color_rgb)), mean_c, istd_c,
                                                x.data_ptr(), m.data_ptr(), H, W, st), "i2r_person_inputs_cv2")
    x._i2r_keep = (tab, list(images))  # the tables / frames must outlive the stream-ordered launch that reads them
    center_dev = tab[off_c:off_s].view(torch.float32).view(S, 2)
    scale_dev = tab[off_s:].view(torch.float32).view(S, 2)
    return x, m, length, center_dev, scale_dev


# ---- the TRAINING half of JointsDataset.__getitem__ (lib/dataset/JointsDataset.py:233-334 with is_train): host geometry in numpy ----
# upper_body_ids of the dataset classes (coco.py:103, crowdpose.py:101, ochuman.py:98), keyed like caller.FLIP_PAIRS
UPPER_BODY_IDS = {
    "coco": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
    "crowdpose": (0, 1, 2, 3, 4, 5, 12, 13),
    "ochuman": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10),
}
# which way half_body_transform went for a person (TrainGeometry.half_body)
HALF_BODY_OFF, HALF_BODY_INELIGIBLE, HALF_BODY_NONE, HALF_BODY_UPPER, HALF_BODY_LOWER = 0, 1, 2, 3, 4


def draw_augmentation(scale_factor, rot_factor, flip, prob_half_body, np_random=np.random, py_random=random):
    """The random draw __getitem__ makes once per IMAGE (JointsDataset.py:237-247; all persons of the image share it)
    -> (rot, sf_ratio, half_flag, flip_flag).  The generators are consumed in the reference's order: py_random.random() <= 0.6 decides
    whether there is a rotation at all and is evaluated FIRST; np_random.randn() for the rotation is consumed only then (clipped to
    [-2 rf, 2 rf]; otherwise rot is the integer 0); randn() for the scale (clipped to [1 - sf, 1 + sf]); rand() < prob_half_body;
    py_random.random() <= 0.5 for the flip only where `flip` is set.  np_random: the numpy.random module or a RandomState; py_random:
    the random module or a random.Random."""
    rf = rot_factor
    rot = np.clip(np_random.randn() * rf, -rf * 2, rf * 2) if py_random.random() <= 0.6 else 0
    sf = scale_factor
    sf_ratio = np.clip(np_random.randn() * sf + 1, 1 - sf, 1 + sf)
    half_flag = bool(np_random.rand() < prob_half_body)
    flip_flag = bool(flip and py_random.random() <= 0.5)
    return rot, sf_ratio, half_flag, flip_flag


def fliplr_joints(joints, joints_vis, width, flip_pairs):
    """lib/utils/transforms.py:33-47 on copies: x = width - x - 1, the pairs of joints and of visibilities swapped, and the joints
    MULTIPLIED by the visibilities (an invisible joint ends at (0, 0, 0)) -> (joints, joints_vis)"""
    j, v = np.array(joints, dtype=np.float64), np.array(joints_vis, dtype=np.float64)
    j[:, 0] = width - j[:, 0] - 1
    for a, b in flip_pairs:
        j[[a, b]] = j[[b, a]]
        v[[a, b]] = v[[b, a]]
    return j * v, v


def half_body_transform(joints, joints_vis, upper_body_ids, aspect_ratio, np_random=np.random, pixel_std=200):
    """JointsDataset.half_body_transform (:71-114) -> (center, scale, branch): float32 centre and scale of the visible upper or lower
    joints, or (None, None, HALF_BODY_NONE) when fewer than two joints are selected.  Quirks kept: the coin is np_random.randn() < 0.5
    (sic: a normal draw, so the upper body is tried 69 % of the time), drawn on every call; the upper body needs MORE than two visible
    joints, else the lower body where it has more than two, else the upper one after all; mean / min / max run in float32; the box is
    widened to the aspect ratio and enlarged by 1.5."""
    upper, lower = [], []
    for j in range(len(joints)):
        if joints_vis[j][0] > 0:
            (upper if j in upper_body_ids else lower).append(joints[j])
    if np_random.randn() < 0.5 and len(upper) > 2:
        sel, branch = upper, HALF_BODY_UPPER
    elif len(lower) > 2:
        sel, branch = lower, HALF_BODY_LOWER
    else:
        sel, branch = upper, HALF_BODY_UPPER
    if len(sel) < 2:
        return None, None, HALF_BODY_NONE
    sel = np.array(sel, dtype=np.float32)
    center = sel.mean(axis=0)[:2]
    lt, rb = np.amin(sel, axis=0), np.amax(sel, axis=0)
    one, ar = np.float32(1), np.float32(aspect_ratio)
    w, h = rb[0] - lt[0] + one, rb[1] - lt[1] + one
    if w > ar * h:
        h = w / ar
    elif w < ar * h:
        w = h * ar
    scale = np.array([w / np.float32(pixel_std), h / np.float32(pixel_std)], dtype=np.float32) * np.float32(1.5)
    return center, scale, branch


def train_affine_transform(center, scale, rot, output_size):
    """get_affine_transform(c, s, r, size) of lib/utils/transforms.py:58-96 with the reference's OWN number formats, which the train
    branch needs to land on the reference's joints to 1e-9 px: scale * 200 and (src_w - 1) * -0.5 stay in the dtype of `scale` (float32
    after half_body_transform, float64 after s * sf_ratio), and get_3rd_point subtracts and adds in FLOAT32 (it gets rows of the float32
    point arrays).  get_affine_transform above does both in float64 and rounds once; the two differ by up to an ulp of a float32 point
    coordinate, 1e-4 px in the map.  cv2.getAffineTransform is the same 3x3 solve in double as there.  -> 2x3 float64"""
    scale = np.asarray(scale)
    dt = scale.dtype.type if scale.dtype in (np.float32, np.float64) else np.float64
    scale_tmp = scale.astype(dt) * dt(200.0)
    half = (scale_tmp[0] - dt(1)) * dt(-0.5)
    dst_w, dst_h = float(output_size[0]), float(output_size[1])
    rot_rad = np.pi * rot / 180
    sn, cs = np.float64(np.sin(rot_rad)), np.float64(np.cos(rot_rad))
    src_dir = np.array([0 * cs - np.float64(half) * sn, 0 * sn + np.float64(half) * cs])
    src = np.zeros((3, 2), dtype=np.float32)
    dst = np.zeros((3, 2), dtype=np.float32)
    c64 = np.asarray(center, dtype=np.float64)
    src[0] = np.asarray(center)
    src[1] = c64 + src_dir
    dst[0] = [(dst_w - 1) * 0.5, (dst_h - 1) * 0.5]
    dst[1] = [(dst_w - 1) * 0.5, (dst_h - 1) * 0.5 + (dst_w - 1) * -0.5]
    for pts in (src, dst):
        d = pts[0] - pts[1]                                          # float32, like get_3rd_point(src[0, :], src[1, :])
        pts[2] = pts[1] + np.array([-d[1], d[0]], dtype=np.float32)
    A = np.concatenate([src.astype(np.float64), np.ones((3, 1))], axis=1)
    return np.linalg.solve(A, dst.astype(np.float64)).T


def rotate_bound_geometry(ih, iw, rot):
    """JointsDataset.rotate_bound (:180-202) without the pixels -> (M, nW, nH): the forward 2x3 map it hands to cv2.warpAffine and the
    size of the canvas it asks for.  M = cv2.getRotationMatrix2D((iw // 2, ih // 2), rot, 1.0) = [[a, b, (1 - a) cx - b cy],
    [-b, a, b cx + (1 - a) cy]] with a = cos, b = sin of the angle; nW = int(ih |b| + iw |a|), nH = int(ih |a| + iw |b|) (truncated);
    then the translation moves by (nW / 2 - cx, nH / 2 - cy) -- half a pixel along every odd dimension already at rot = 0."""
    cx, cy = iw // 2, ih // 2
    ang = rot * (np.pi / 180.0)                                          # (imgwarp.cpp: angle *= CV_PI / 180)
    a, b = float(np.cos(ang)), float(np.sin(ang))
    M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)
    cos, sin = np.abs(M[0, 0]), np.abs(M[0, 1])
    nW, nH = int(ih * sin + iw * cos), int(ih * cos + iw * sin)
    M[0, 2] += nW / 2 - cx
    M[1, 2] += nH / 2 - cy
    return M, nW, nH


class TrainGeometry:
    """train_geometry's result for ONE image of n persons: what __getitem__ returns beside the pixels, and what the pixels need.
    rotation, sf_ratio, half_flag, flip: the draw; trans / trans_heatmap [n, 2, 3] float64: the forward maps of the crops;
    center, scale [n, 2] float64 (meta['center'], meta['scale']); joints [n, J, 3] float64 (meta['joints']: x, y in the INPUT crop where
    visible, the flipped image's coordinates -- (0, 0) after a flip -- where not); joints_hm [n, J, 3] float64 (the joints_heatmap that
    generate_target gets); joints_vis [n, J, 3] float64; half_body int [n] (HALF_BODY_*); box int32 [n, 4]: the inclusive corners
    cv2.rectangle fills, in the UNFLIPPED image; mask_trans 2x3, canvas (nW, nH): rotate_bound_geometry; image_shape (ih, iw)."""
    __slots__ = ("rotation", "sf_ratio", "half_flag", "flip", "trans", "trans_heatmap", "center", "scale", "joints", "joints_hm",
                 "joints_vis", "half_body", "box", "mask_trans", "canvas", "image_shape")


def train_geometry(annos, draw, image_shape, image_size, heatmap_size, flip_pairs, upper_body_ids, num_joints_half_body=8,
                   np_random=np.random):
    """The train branch of __getitem__ for one image (JointsDataset.py:269-323), everything but the pixels, in the reference's order
    and number formats.  annos: the image's db records, each with 'joints_3d', 'joints_3d_vis' [J, 3], 'center', 'scale' (2,) and
    'box' (x, y, w, h); nothing is modified.  draw: draw_augmentation's tuple.  image_shape = (ih, iw); image_size / heatmap_size =
    (W, H) / (w, h).  Per person: fliplr_joints and c[0] = iw - c[0] - 1 (in the dtype of the centre) where the image is flipped;
    s * sf_ratio (the float64 draw promotes a float32 scale to float64, as numpy >= 2 does for the reference's own line);
    half_body_transform where sum(vis) > num_joints_half_body and the flag is set (its own np_random.randn() is consumed then, a None
    result keeps c, s); the two maps; the joints moved where vis > 0.  -> TrainGeometry"""
    rot, sf_ratio, half_flag, flip = draw
    ih, iw = int(image_shape[0]), int(image_shape[1])
    aspect = float(image_size[0]) * 1.0 / float(image_size[1])
    g = TrainGeometry()
    g.rotation, g.sf_ratio, g.half_flag, g.flip, g.image_shape = rot, sf_ratio, bool(half_flag), bool(flip), (ih, iw)
    n = len(annos)
    assert n >= 1
    tr, trh, cen, scl, jts, jhm, jvs, hb, box = [], [], [], [], [], [], [], [], []
    for anno in annos:
        joints = np.array(anno["joints_3d"], dtype=np.float64)
        vis = np.array(anno["joints_3d_vis"], dtype=np.float64)
        c, s = np.array(anno["center"]), np.array(anno["scale"])
        if c.dtype not in (np.float32, np.float64):
            c = c.astype(np.float64)
        if flip:
            joints, vis = fliplr_joints(joints, vis, iw, flip_pairs)
            c[0] = iw - c[0] - 1
        s = s.astype(np.float64) * np.float64(sf_ratio)
        branch = HALF_BODY_OFF
        if half_flag:
            branch = HALF_BODY_INELIGIBLE
            if np.sum(vis[:, 0]) > num_joints_half_body:
                c_hb, s_hb, branch = half_body_transform(joints, vis, upper_body_ids, aspect, np_random)
                if c_hb is not None:
                    c, s = c_hb, s_hb
        t = train_affine_transform(c, s, rot, image_size)
        th = train_affine_transform(c, s, rot, heatmap_size)
        joints_hm = joints.copy()
        for j in range(joints.shape[0]):
            if vis[j, 0] > 0.0:
                pt = np.array([joints[j, 0], joints[j, 1], 1.0])
                joints[j, 0:2] = np.dot(t, pt)
                joints_hm[j, 0:2] = np.dot(th, pt)
        x, y, w, h = [float(v) for v in anno["box"][:4]]
        tr.append(t), trh.append(th), cen.append(np.asarray(c, np.float64)), scl.append(np.asarray(s, np.float64))
        jts.append(joints), jhm.append(joints_hm), jvs.append(vis), hb.append(branch)
        box.append([int(x), int(y), int(x + w), int(y + h)])   # cv2.rectangle's corners: int() truncates (JointsDataset.py:169-170)
    g.trans, g.trans_heatmap, g.center, g.scale = np.stack(tr), np.stack(trh), np.stack(cen), np.stack(scl)
    g.joints, g.joints_hm, g.joints_vis = np.stack(jts), np.stack(jhm), np.stack(jvs)
    g.half_body = np.asarray(hb, dtype=np.int32)
    g.box = np.clip(np.asarray(box, dtype=np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    g.mask_trans, nW, nH = rotate_bound_geometry(ih, iw, rot)
    g.canvas = (nW, nH)
    return g


_TRAIN_CROP_DT = np.dtype([("inv_m", "<f8", 6), ("mask_inv_m", "<f8", 6), ("box", "<i4", 4), ("nw", "<i4"), ("nh", "<i4"), ("image", "<i4"),
                           ("flip", "<i4"), ("reserved", "<i4", 4)])   # i2r_train_crop_ref, 144 bytes
assert _TRAIN_CROP_DT.itemsize == 144


class TrainInputs:
    """train_inputs_batch's result.  Device tensors: x [S, 3, H, W] and pos_mask [S, 1, H, W] fp32 (the collated input_list /
    pos_mask_list after ToTensor / Normalize); joints_hm float64 [S, J, 2] and joints_vis fp32 [S, J]: the analytic target form of
    caller.val_metrics / head_grad / HeadFit.step; joints float64 [S, J, 2] (meta['joints']); center, scale fp32 [S, 2].  Host: length
    (persons per image), rotation and flip (one per image), geometry (the TrainGeometry of every image)."""
    __slots__ = ("x", "pos_mask", "length", "joints_hm", "joints_vis", "joints", "center", "scale", "rotation", "flip", "geometry", "_i2r_keep")


def train_inputs_batch(images, annos, draws, image_size, heatmap_size, dataset="coco", color_rgb=False, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                       device="cuda:0", flip_pairs=None, upper_body_ids=None, num_joints_half_body=8, np_random=np.random, geometry=None):
    """The TRAINING samples of a batch of images on the device: what JointsDataset.__getitem__ with is_train builds per person with
    cv2 -- crop of the (flipped) image under the rotated, rescaled, possibly half-body map, the box mask after rotate_bound(mask, r) and
    cv2.resize -- plus the joints for the analytic targets, in ONE launch (i2r_train_inputs_cv2) and ONE pinned, stream-ordered upload.
    images: uint8 [ih_i, iw_i, 3] tensors on `device` (unflipped: the kernel mirrors); annos: per image the list of db records
    (train_geometry); draws: per image draw_augmentation's tuple.  dataset keys caller.FLIP_PAIRS / UPPER_BODY_IDS unless flip_pairs /
    upper_body_ids are given.  The half-body coin of every eligible person is drawn from np_random image after image; to consume the
    generators exactly as a loop over the reference's __getitem__ would, interleave draw_augmentation and train_geometry per image
    yourself and hand the results in as geometry= (draws is ignored then).  cv2's fixed-point arithmetic.  -> TrainInputs"""
    from . import caller
    dev = torch.device(device)
    W, H = int(image_size[0]), int(image_size[1])
    flip_pairs = caller.FLIP_PAIRS[dataset] if flip_pairs is None else flip_pairs
    upper_body_ids = UPPER_BODY_IDS[dataset] if upper_body_ids is None else upper_body_ids
    n_img = len(images)
    for im in images:
        assert im.is_cuda and im.device == dev and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3 and im.is_contiguous()
    if geometry is None:
        assert len(annos) == n_img == len(draws)
        geometry = [train_geometry(annos[i], draws[i], images[i].shape[:2], (W, H), heatmap_size, flip_pairs, upper_body_ids,
                                   num_joints_half_body, np_random) for i in range(n_img)]
    assert len(geometry) == n_img and all(tuple(g.image_shape) == tuple(images[i].shape[:2]) for i, g in enumerate(geometry))
    length = [len(g.trans) for g in geometry]
    S = sum(length)
    J = geometry[0].joints.shape[1]
    assert S >= 1 and all(g.joints.shape[1] == J for g in geometry)
    # one host buffer: [crop table | image table | joints_hm f64 | joints f64 | joints_vis f32 | centres f32 | scales f32]
    off_img = S * 144
    off_hm = off_img + (n_img * 24 + 15) // 16 * 16
    off_j = off_hm + S * J * 16
    off_v = off_j + S * J * 16
    off_c = off_v + (S * J * 4 + 15) // 16 * 16
    off_s = off_c + S * 8
    host = torch.empty(off_s + S * 8, dtype=torch.uint8).pin_memory()
    hb = host.numpy()
    hb[:] = 0
    crops = hb[:off_img].view(_TRAIN_CROP_DT)
    crops["inv_m"] = cv2_inverse_batch(np.concatenate([g.trans for g in geometry]))
    crops["mask_inv_m"] = np.repeat(np.stack([cv2_inverse(g.mask_trans).reshape(6) for g in geometry]), length, axis=0)
    boxes = np.concatenate([g.box for g in geometry]).astype(np.int64)
    iw_p = np.repeat([g.image_shape[1] for g in geometry], length)
    ih_p = np.repeat([g.image_shape[0] for g in geometry], length)
    # clipped to the image: cv2.rectangle draws nothing outside it (a box wholly outside ends with x0 > x1 or y0 > y1: nothing is set)
    crops["box"] = np.stack([np.maximum(boxes[:, 0], 0), np.maximum(boxes[:, 1], 0), np.minimum(boxes[:, 2], iw_p - 1),
                             np.minimum(boxes[:, 3], ih_p - 1)], 1).astype(np.int32)
    crops["nw"] = np.repeat([g.canvas[0] for g in geometry], length)
    crops["nh"] = np.repeat([g.canvas[1] for g in geometry], length)
    crops["image"] = np.repeat(np.arange(n_img, dtype=np.int32), length)
    crops["flip"] = np.repeat([int(g.flip) for g in geometry], length)
    imgs = hb[off_img:off_img + n_img * 24].view(_IMG_DT)
    for i, im in enumerate(images):
        imgs[i] = (im.data_ptr(), im.shape[0], im.shape[1], im.shape[1] * 3, 0)
    hb[off_hm:off_j].view(np.float64)[:] = np.concatenate([g.joints_hm[:, :, :2] for g in geometry]).reshape(-1)
    hb[off_j:off_j + S * J * 16].view(np.float64)[:] = np.concatenate([g.joints[:, :, :2] for g in geometry]).reshape(-1)
    hb[off_v:off_v + S * J * 4].view(np.float32)[:] = np.concatenate([g.joints_vis[:, :, 0] for g in geometry]).astype(np.float32).reshape(-1)
    hb[off_c:off_s].view(np.float32)[:] = np.concatenate([g.center for g in geometry]).astype(np.float32).reshape(-1)
    hb[off_s:].view(np.float32)[:] = np.concatenate([g.scale for g in geometry]).astype(np.float32).reshape(-1)
    tab = host.to(dev, non_blocking=True)
    r = TrainInputs()
    r.x = torch.empty(S, 3, H, W, dtype=torch.float32, device=dev)
    r.pos_mask = torch.empty(S, 1, H, W, dtype=torch.float32, device=dev)
    mean_c = (C.c_float * 3)(*mean)
    istd_c = (C.c_float * 3)(*[1.0 / v for v in std])
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        cabi.check(cabi.lib().i2r_train_inputs_cv2(tab.data_ptr() + off_img, n_img, tab.data_ptr(), S, int(bool(color_rgb)), mean_c, istd_c,
                                                   r.x.data_ptr(), r.pos_mask.data_ptr(), H, W, st), "i2r_train_inputs_cv2")
    r._i2r_keep = r.x._i2r_keep = (tab, list(images), host)  # the tables / frames must outlive the stream-ordered launch that reads them
    r.length = length
    r.joints_hm = tab[off_hm:off_j].view(torch.float64).view(S, J, 2)
    r.joints = tab[off_j:off_j + S * J * 16].view(torch.float64).view(S, J, 2)
    r.joints_vis = tab[off_v:off_v + S * J * 4].view(torch.float32).view(S, J)
    r.center = tab[off_c:off_s].view(torch.float32).view(S, 2)
    r.scale = tab[off_s:].view(torch.float32).view(S, 2)
    r.rotation, r.flip, r.geometry = [g.rotation for g in geometry], [g.flip for g in geometry], list(geometry)
    return r


def collate(batch):
    """collater.__call__ with max_patch = 0 (tools/test.py:139; lib/dataset/collater.py:14-26,175-183) for the two tensors the
    forward consumes: batch = [(input_list_i, pos_mask_list_i), ...] per image, each a list of per-person tensors or a stacked
    [n_i, ...] tensor -> (input [S,3,H,W], pos_mask [S,1,H,W], length)."""
    xs, ms, length = [], [], []
    for inp, msk in batch:
        inp = torch.stack(list(inp), dim=0) if not torch.is_tensor(inp) else inp
        msk = torch.stack(list(msk), dim=0) if not torch.is_tensor(msk) else msk
        assert inp.shape[0] == msk.shape[0]
        xs.append(inp)
        ms.append(msk)
        length.append(int(inp.shape[0]))
    return torch.cat(xs), torch.cat(ms), length


# ---- grouped test modes of the reference's collater (lib/dataset/collater.py:28-95 with DATASET.MAX_PATCH > 0) ----
def window_lengths(length, max_patch):
    """PATCH_MODE window (collater.py:68-91, extend_list): an image of more than max_patch persons is cut into consecutive chunks of
    max_patch, the last one shorter.  The crops keep their order, so model(x, pos_mask, window_lengths(length, max_patch)) IS that mode."""
    p = int(max_patch)
    if p < 1:
        raise ValueError("max_patch must be >= 1 (got %r)" % (max_patch,))
    out = []
    for n in length:
        n = int(n)
        out += [min(p, n - i) for i in range(0, n, p)] if n > p else [n]
    return out


def group_layout(length, max_patch):
    """What the main_target grouping of a batch looks like, from the person counts alone: -> (group_len, person_off, member_off).  An
    image of one person is one group of one; an image of n > 1 persons gives n groups of min(n, max_patch) members (collater.py:35-51).
    group_len: members of every group, target by target (one group per person of the batch); person_off / member_off: the images' first
    persons and first slots in the member table, [images + 1] each."""
    p = int(max_patch)
    if p < 1:
        raise ValueError("max_patch must be >= 1 (got %r)" % (max_patch,))
    group_len, person_off, member_off = [], [0], [0]
    for n in length:
        n = int(n)
        if n < 1:
            raise ValueError("every image needs at least one person (length %r)" % (list(length),))
        k = 1 if n == 1 else min(n, p)
        group_len += [k] * n
        person_off.append(person_off[-1] + n)
        member_off.append(member_off[-1] + n * k)
    return group_len, person_off, member_off


MAX_PATCH_LIMIT = 64  # i2r_group_nearest (include/i2r_hip.h)


class PersonGroups:
    """main_target_groups' result: members = device int32 [sum(group_len)] of global crop indices, group after group, every group's
    target first; group_len = host list, one group per person of the batch in input order; n_groups = len(group_len)."""
    __slots__ = ("members", "group_len", "n_groups", "_keep")

    def __init__(self, members, group_len, keep=None):
        self.members, self.group_len, self.n_groups, self._keep = members, list(group_len), len(group_len), keep


def main_target_groups(boxes, length, max_patch, device="cuda:0"):
    """PATCH_MODE main_target (collater.py:35-51): one group per person -- the person itself, then its min(n, max_patch) - 1 nearest
    neighbours in the image by the distance between the boxes' top-left corners (i2r_group_nearest; equal distances: the lower index
    first; the target always first, also where another person shares its corner).  boxes: [S, >= 2] (x, y, ...) per crop in batch order,
    a host array or a device tensor of any float type; length: persons per image.  -> PersonGroups; nothing is read back from the device."""
    dev = torch.device(device)
    group_len, person_off, member_off = group_layout(length, max_patch)
    if int(max_patch) > MAX_PATCH_LIMIT:
        raise ValueError("max_patch %d: at most %d" % (int(max_patch), MAX_PATCH_LIMIT))
    S, n_members, B = person_off[-1], member_off[-1], len(person_off) - 1
    b = boxes if torch.is_tensor(boxes) else torch.from_numpy(np.asarray(boxes, dtype=np.float64).reshape(S, -1))
    if b.dim() != 2 or b.shape[0] != S or b.shape[1] < 2 or not b.is_floating_point():
        raise ValueError("boxes: shape %s %s, expected floating point [%d, >= 2]" % (tuple(b.shape), b.dtype, S))
    anchors = b[:, :2].to(dev, torch.float64).contiguous()
    offs = torch.tensor(person_off + member_off, dtype=torch.int32).to(dev)
    members = torch.empty(n_members, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        cabi.check(cabi.lib().i2r_group_nearest(anchors.data_ptr(), offs.data_ptr(), offs.data_ptr() + 4 * (B + 1), B, S, n_members, int(max_patch),
                                                members.data_ptr(), st), "i2r_group_nearest")
    return PersonGroups(members, group_len, keep=(anchors, offs))  # (the tables must outlive the stream-ordered launch that reads them)
