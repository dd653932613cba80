"""The training samples of JointsDataset.__getitem__ (lib/dataset/JointsDataset.py:233-334) the slow way, for tests/test_train_inputs.py
and tests/test_train_inputs_gpu.py: every intermediate image is MATERIALISED -- the mirrored image, the filled rectangle, the mirrored
rectangle, rotate_bound's nW x nH canvas -- and pushed through oracle/input_cpu.py (cv2_warp_affine, cv2_resize_linear_u8).  It shares no
code with the kernel's canvas-free form (csrc/i2r_input.hip train_mask_pixel_cv2) nor with input.rotate_bound_geometry.  Plus the loader
of tests/golden/train_inputs_reference.npz (tools/make_golden_train_inputs.py: the reference's own __getitem__) and the replay of a
fixture sample through the host functions of i2r_amd.input."""
import functools
import os
import random
import types

import numpy as np

import _input_cases
import input_cpu
from i2r_amd import input as inp

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_inputs_reference.npz")


def rectangle(ih, iw, box_int, flip):
    """get_position(shape, box, 'single', flipFlag): cv2.rectangle filled with 255 between inclusive corners, then [:, ::-1]"""
    x0, y0, x1, y1 = [int(v) for v in box_int]
    m = np.zeros((ih, iw), dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x1, iw - 1), max(y0, 0), min(y1, ih - 1)
    if xa <= xb and ya <= yb:
        m[ya:yb + 1, xa:xb + 1] = 255
    return np.ascontiguousarray(m[:, ::-1]) if flip else m


def rotate_bound(image, angle):
    """JointsDataset.rotate_bound on a real image: the canvas, uint8 [nH, nW]"""
    h, w = image.shape[:2]
    cx, cy = w // 2, h // 2
    th = np.deg2rad(angle)
    a, b = np.cos(th), np.sin(th)
    M = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])
    nW, nH = int(h * abs(b) + w * abs(a)), int(h * abs(a) + w * abs(b))
    M[0, 2] += nW / 2 - cx
    M[1, 2] += nH / 2 - cy
    return input_cpu.cv2_warp_affine(image, M, (nW, nH))


def materialised(img, trans, boxes_int, rot, flip, size, swap_rb=False):
    """img uint8 [ih, iw, 3], trans [n, 2, 3] forward maps, boxes_int [n, 4] inclusive corners in the unflipped image, size (W, H)
    -> (crops uint8 [n, H, W, 3], masks uint8 [n, H, W])"""
    W, H = size
    ih, iw = img.shape[:2]
    src = np.ascontiguousarray(img[:, ::-1]) if flip else np.ascontiguousarray(img)
    if swap_rb:
        src = np.ascontiguousarray(src[:, :, ::-1])
    crops = np.stack([input_cpu.cv2_warp_affine(src, t, (W, H)) for t in trans])
    masks = np.stack([input_cpu.cv2_resize_linear_u8(rotate_bound(rectangle(ih, iw, b, flip), rot), (W, H)) for b in boxes_int])
    return crops, masks


def normalised(crops_u8, mean=inp.IMAGENET_MEAN, std=inp.IMAGENET_STD):
    """uint8 [n, H, W, 3] -> fp32 [n, 3, H, W]: ToTensor + Normalize in fp32, as the kernels round it"""
    x = crops_u8.transpose(0, 3, 1, 2).astype(np.float32) * np.float32(1.0 / 255.0)
    m = np.asarray(mean, np.float32)[None, :, None, None]
    s = np.asarray([1.0 / v for v in std], np.float32)[None, :, None, None]
    return (x - m) * s


@functools.lru_cache(maxsize=None)
def fixture():
    """-> namespace: sets (list of namespaces: name, image, image_size, heatmap_size, flip_pairs, upper_body_ids, annos), samples (list
    of namespaces with the recorded arrays), scale_factor, rot_factor, prob_half_body, sigma"""
    z = np.load(FIXTURE)
    f = types.SimpleNamespace(scale_factor=float(z["scale_factor"]), rot_factor=int(z["rot_factor"]), prob_half_body=float(z["prob_half_body"]),
                              sigma=int(z["sigma"]), sets=[], samples=[])
    for si, name in enumerate(z["set_names"]):
        q = "set%d_" % si
        ih, iw = [int(v) for v in z[q + "image_shape"]]
        img = _input_cases.image(str(z[q + "image_kind"]), ih, iw)
        assert int(img.astype(np.int64).sum()) == int(z[q + "image_sum"]), "the regenerated image is the one the reference saw"
        n = z[q + "box"].shape[0]
        annos = [dict(joints_3d=z[q + "joints_3d"][p], joints_3d_vis=z[q + "joints_3d_vis"][p], center=z[q + "center"][p], scale=z[q + "scale"][p],
                      box=z[q + "box"][p]) for p in range(n)]
        for a in annos:
            for v in a.values():
                v.setflags(write=False)
        f.sets.append(types.SimpleNamespace(name=str(name), image=img, image_size=tuple(int(v) for v in z[q + "image_size"]),
                                            heatmap_size=tuple(int(v) for v in z[q + "heatmap_size"]), flip_pairs=z[q + "flip_pairs"].tolist(),
                                            upper_body_ids=tuple(int(v) for v in z[q + "upper_body_ids"]), annos=annos))
    keys = ("seed", "set", "njhb", "rot", "rot_is_int", "sf_ratio", "half_flag", "flip", "half_body", "next_py", "next_np", "crops", "masks",
            "target_weight", "joints_hm", "joints", "joints_vis", "center", "scale", "scale_is_f32", "center_is_f32")
    for i in range(int(z["n_samples"])):
        s = types.SimpleNamespace(**{k: z["s%d_%s" % (i, k)] for k in keys})
        for k in ("seed", "set", "njhb"):
            setattr(s, k, int(getattr(s, k)))
        for k in ("rot_is_int", "half_flag", "flip"):
            setattr(s, k, bool(getattr(s, k)))
        f.samples.append(s)
    return f


def replay(i):
    """fixture sample i through input.draw_augmentation + input.train_geometry from its seed
    -> (draw, TrainGeometry, the next values of the two generators)"""
    f = fixture()
    s = f.samples[i]
    st = f.sets[s.set]
    py, npr = random.Random(s.seed), np.random.RandomState(s.seed)
    draw = inp.draw_augmentation(f.scale_factor, f.rot_factor, True, f.prob_half_body, np_random=npr, py_random=py)
    g = inp.train_geometry(st.annos, draw, st.image.shape[:2], st.image_size, st.heatmap_size, st.flip_pairs, st.upper_body_ids,
                           num_joints_half_body=s.njhb, np_random=npr)
    return draw, g, (py.random(), npr.rand())
