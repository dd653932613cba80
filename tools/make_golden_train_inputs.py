"""Generate tests/golden/train_inputs_reference.npz by running THE REFERENCE'S OWN JointsDataset.__getitem__ with is_train=True and
transform=None (lib/dataset/JointsDataset.py:207-356: crops and masks stay uint8) on synthetic images and annotations.
Run where the reference exists (oracle/ref_shim.py REF_ROOT):

    python tools/make_golden_train_inputs.py

The control flow, the random draws, fliplr_joints, half_body_transform, get_affine_transform, affine_transform, rotate_bound and
generate_target are the reference's.  THE PIXEL ARITHMETIC IS NOT REAL cv2: cv2 is absent here, so `cv2` is a stand-in module whose
getAffineTransform (a 3x3 solve in double), warpAffine, rectangle, getRotationMatrix2D and resize delegate to the restatement of
OpenCV's published algorithm in oracle/input_cpu.py, and whose imread hands back the synthetic image.  What this fixture pins is
therefore the reference's geometry, order and number formats, and the composition of the restated pixel steps -- not a cv2 output.

Two data sets: 17 joints with the COCO pairs on a 97 x 131 smooth image, output 48 x 64, heat map 12 x 16; 14 joints with the CrowdPose
pairs on a 96 x 130 noise image, output 17 x 23, heat map 5 x 6.  Three persons per image: one with most joints visible, one whose box
sticks out of the image and who has three visible joints, one with a visible lower body.  SCALE_FACTOR 0.3, ROT_FACTOR 40,
PROB_HALF_BODY 0.5, NUM_JOINTS_HALF_BODY 8 or 2 (at 2 the three-joint person reaches half_body_transform and gets None back).
Seeds are taken in ascending order while they add something to the coverage list asserted at the end (COVER).  The draws are read from
the locals of the running __getitem__ frame; joints_heatmap by wrapping generate_target on the instance; the half-body branch by
wrapping half_body_transform and comparing its centre with the float32 means of the two joint sets.  Data only."""
import importlib.util
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import input_cpu  # noqa: E402
from ref_shim import REF_LIB  # noqa: E402

SCALE_FACTOR, ROT_FACTOR, PROB_HALF_BODY, SIGMA = 0.3, 40, 0.5, 2
COCO_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]          # coco.py:100-101
CROWDPOSE_PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]]                          # crowdpose.py:98-99
SETS = [  # name, J, pairs, upper_body_ids, image kind, (ih, iw), image_size (W, H), heatmap_size (w, h)
    ("coco", 17, COCO_PAIRS, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10), "smooth", (97, 131), (48, 64), (12, 16)),
    ("crowdpose", 14, CROWDPOSE_PAIRS, (0, 1, 2, 3, 4, 5, 12, 13), "noise", (96, 130), (17, 23), (5, 6)),
]
COVER = ("rot0", "rot", "rot_clip_lo", "rot_clip_hi", "sf_clip_lo", "sf_clip_hi", "flip", "noflip", "hb_upper", "hb_lower", "hb_none",
         "hb_ineligible", "hb_off", "box_out", "J17", "J14", "coco_flip", "crowdpose_flip", "coco_rot", "crowdpose_rot", "coco_rot0",
         "crowdpose_rot0", "flip_rot_hb")
MAX_SAMPLES = 12
HB_OFF, HB_INELIGIBLE, HB_NONE, HB_UPPER, HB_LOWER = 0, 1, 2, 3, 4


def make_cv2(images):
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_COLOR, cv2.IMREAD_IGNORE_ORIENTATION, cv2.INTER_LINEAR, cv2.COLOR_BGR2RGB = 1, 128, 1, 4

    def imread(path, flags=None):
        return images[path].copy()

    def getAffineTransform(src, dst):
        A = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], axis=1)
        return np.linalg.solve(A, np.asarray(dst, np.float64)).T

    def warpAffine(img, M, dsize, flags=None):
        return input_cpu.cv2_warp_affine(np.ascontiguousarray(img), M, (int(dsize[0]), int(dsize[1])))

    def rectangle(img, pt1, pt2, color, thickness):
        assert thickness == -1 and pt1[0] <= pt2[0] and pt1[1] <= pt2[1]
        ih, iw = img.shape[:2]
        xa, xb, ya, yb = max(pt1[0], 0), min(pt2[0], iw - 1), max(pt1[1], 0), min(pt2[1], ih - 1)
        if xa <= xb and ya <= yb:
            img[ya:yb + 1, xa:xb + 1] = color
        return img

    def getRotationMatrix2D(center, angle, scale):
        ang = angle * (np.pi / 180.0)                                 # (imgwarp.cpp: angle *= CV_PI / 180)
        a, b = np.cos(ang) * scale, np.sin(ang) * scale
        return np.array([[a, b, (1 - a) * center[0] - b * center[1]], [-b, a, b * center[0] + (1 - a) * center[1]]], dtype=np.float64)

    def resize(src, dsize):
        return input_cpu.cv2_resize_linear_u8(np.ascontiguousarray(src), (int(dsize[0]), int(dsize[1])))

    cv2.imread, cv2.getAffineTransform, cv2.warpAffine, cv2.rectangle = imread, getAffineTransform, warpAffine, rectangle
    cv2.getRotationMatrix2D, cv2.resize = getRotationMatrix2D, resize
    return cv2


def import_reference(images):
    sys.modules["cv2"] = make_cv2(images)
    for name in ("matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Compose = lambda steps: None          # mask_transform: built in __init__, never called with transform=None
    tv.transforms.ToTensor = lambda: None
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    sys.path.insert(0, REF_LIB)
    spec = importlib.util.spec_from_file_location("ref_JointsDataset", os.path.join(REF_LIB, "dataset", "JointsDataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.JointsDataset


def box_to_center_scale(box, image_size):
    """_box2cs / _xywh2cs of the dataset classes (coco.py, crowdpose.py): float32 centre and scale"""
    x, y, w, h = box
    aspect = image_size[0] * 1.0 / image_size[1]
    center = np.zeros(2, dtype=np.float32)
    center[0], center[1] = x + (w - 1) * 0.5, y + (h - 1) * 0.5
    if w > aspect * h:
        h = w * 1.0 / aspect
    elif w < aspect * h:
        w = h * aspect
    return center, np.array([w * 1.0 / 200, h * 1.0 / 200], dtype=np.float32) * 1.25


def make_annos(si, J, upper_ids, ih, iw, image_size):
    """three persons: 0 = most joints visible, inside; 1 = box out of the image at the right / bottom, one upper and two lower joints
    visible; 2 = two upper joints and the whole lower body visible"""
    rng = np.random.RandomState(100 + si)
    lower_ids = [j for j in range(J) if j not in upper_ids]
    boxes = [(0.12 * iw + 0.37, 0.1 * ih + 0.21, 0.45 * iw, 0.7 * ih), (0.7 * iw + 0.6, 0.55 * ih + 0.3, 0.5 * iw, 0.6 * ih),
             (0.4 * iw + 0.11, 0.3 * ih + 0.77, 0.3 * iw, 0.5 * ih)]
    annos = []
    for p, box in enumerate(boxes):
        x, y, w, h = box
        joints = np.zeros((J, 3), dtype=np.float64)
        joints[:, 0] = np.clip(rng.uniform(x, x + w, J), 0, iw - 1)
        joints[:, 1] = np.clip(rng.uniform(y, y + h, J), 0, ih - 1)
        joints[list(upper_ids) + lower_ids, 1] = np.sort(joints[:, 1])   # upper-body joints higher in the image: the two halves differ
        vis = np.zeros((J, 3), dtype=np.float64)
        if p == 0:
            vis[:, :2] = 1
            vis[[upper_ids[1], lower_ids[0]], :2] = 0
        elif p == 1:
            vis[[upper_ids[2], lower_ids[1], lower_ids[2]], :2] = 1
        else:
            vis[list(lower_ids) + [upper_ids[0], upper_ids[3]], :2] = 1
        joints[vis[:, 0] == 0] = 0                                    # as the dataset classes leave unlabelled joints
        c, s = box_to_center_scale(box, image_size)
        annos.append(dict(joints_3d=joints, joints_3d_vis=vis, center=c, scale=s, box=np.array(box, dtype=np.float64), imgnum=p))
    return annos


def features(rec, name):
    f = {name + ("_rot" if rec["rot"] != 0 else "_rot0"), "rot" if rec["rot"] != 0 else "rot0", "flip" if rec["flip"] else "noflip",
         "J17" if name == "coco" else "J14", "box_out"}
    if rec["flip"]:
        f.add(name + "_flip")
    if rec["rot"] == -2 * ROT_FACTOR:
        f.add("rot_clip_lo")
    if rec["rot"] == 2 * ROT_FACTOR:
        f.add("rot_clip_hi")
    if rec["sf_ratio"] == 1 - SCALE_FACTOR:
        f.add("sf_clip_lo")
    if rec["sf_ratio"] == 1 + SCALE_FACTOR:
        f.add("sf_clip_hi")
    f |= {{HB_OFF: "hb_off", HB_INELIGIBLE: "hb_ineligible", HB_NONE: "hb_none", HB_UPPER: "hb_upper", HB_LOWER: "hb_lower"}[b] for b in rec["half_body"]}
    if rec["flip"] and rec["rot"] != 0 and (HB_UPPER in rec["half_body"] or HB_LOWER in rec["half_body"]):
        f.add("flip_rot_hb")
    return f


def run_sample(ds, JointsDataset, seed, upper_ids):
    """one __getitem__(0) from freshly seeded generators -> dict of what the reference computed"""
    rec = {"hb": []}

    def generate_target(joints_heatmap, joints_vis):
        fr = sys._getframe(1).f_locals                                # the running __getitem__: its draws
        rec["draw"] = (fr["r"], fr["sf_ratio"], bool(fr["half_trans_flag"]), bool(fr["flipFlag"]))
        rec.setdefault("joints_hm", []).append(np.array(joints_heatmap, dtype=np.float64))
        rec["hb"].append(rec.pop("hb_now", HB_INELIGIBLE if fr["half_trans_flag"] else HB_OFF))
        return JointsDataset.generate_target(ds, joints_heatmap, joints_vis)

    def half_body_transform(joints, joints_vis):
        c, s = JointsDataset.half_body_transform(ds, joints, joints_vis)
        if c is None:
            rec["hb_now"] = HB_NONE
        else:
            means = {}
            for tag, ids in ((HB_UPPER, upper_ids), (HB_LOWER, [j for j in range(ds.num_joints) if j not in upper_ids])):
                sel = [joints[j] for j in ids if joints_vis[j][0] > 0]
                means[tag] = np.array(sel, dtype=np.float32).mean(axis=0)[:2] if sel else None
            hit = [tag for tag, m in means.items() if m is not None and np.array_equal(m, c)]
            assert len(hit) == 1, hit
            rec["hb_now"] = hit[0]
        return c, s

    ds.generate_target, ds.half_body_transform = generate_target, half_body_transform
    random.seed(seed)
    np.random.seed(seed)
    input_list, pos_mask_list, target_list, target_weight_list, meta = ds[0]
    out = dict(seed=seed, rot=rec["draw"][0], sf_ratio=rec["draw"][1], half_flag=rec["draw"][2], flip=rec["draw"][3],
               rot_is_int=isinstance(rec["draw"][0], int), half_body=np.asarray(rec["hb"], np.int32),
               next_py=random.random(), next_np=np.random.rand(),
               crops=np.stack(input_list), masks=np.stack(pos_mask_list),
               target_weight=np.stack([t.numpy() for t in target_weight_list])[:, :, 0], joints_hm=np.stack(rec["joints_hm"]),
               joints=np.stack(meta["joints"]).astype(np.float64), joints_vis=np.stack(meta["joints_vis"]).astype(np.float64),
               center=np.stack([np.asarray(c, np.float64) for c in meta["center"]]),
               scale=np.stack([np.asarray(s, np.float64) for s in meta["scale"]]),
               scale_is_f32=np.asarray([np.asarray(s).dtype == np.float32 for s in meta["scale"]]),
               center_is_f32=np.asarray([np.asarray(c).dtype == np.float32 for c in meta["center"]]))
    assert out["crops"].dtype == np.uint8 and out["masks"].dtype == np.uint8 and meta["rotation"] == out["rot"]
    return out


def main():
    import _input_cases
    import torch
    images = {}
    JointsDataset = import_reference(images)
    data = {"numpy_version": np.asarray(np.__version__), "torch_version": np.asarray(torch.__version__), "scale_factor": np.float64(SCALE_FACTOR),
            "rot_factor": np.int32(ROT_FACTOR), "prob_half_body": np.float64(PROB_HALF_BODY), "sigma": np.int32(SIGMA),
            "set_names": np.asarray([s[0] for s in SETS])}
    covered, samples = set(), []
    cand = []
    for si, (name, J, pairs, upper_ids, kind, (ih, iw), image_size, heatmap_size) in enumerate(SETS):
        img = _input_cases.image(kind, ih, iw)
        images[name] = np.array(img)
        annos = make_annos(si, J, upper_ids, ih, iw, image_size)
        q = "set%d_" % si
        data[q + "image_kind"], data[q + "image_shape"], data[q + "image_sum"] = np.asarray(kind), np.asarray([ih, iw], np.int32), np.int64(img.astype(np.int64).sum())
        data[q + "image_size"], data[q + "heatmap_size"] = np.asarray(image_size, np.int32), np.asarray(heatmap_size, np.int32)
        data[q + "flip_pairs"], data[q + "upper_body_ids"] = np.asarray(pairs, np.int32), np.asarray(upper_ids, np.int32)
        for k in ("joints_3d", "joints_3d_vis", "center", "scale", "box"):
            data[q + k] = np.stack([a[k] for a in annos])
        for njhb in (8, 2):
            cfg = types.SimpleNamespace(
                OUTPUT_DIR="", LOSS=types.SimpleNamespace(USE_DIFFERENT_JOINTS_WEIGHT=False),
                DATASET=types.SimpleNamespace(DATA_FORMAT="jpg", SCALE_FACTOR=SCALE_FACTOR, ROT_FACTOR=ROT_FACTOR, FLIP=True,
                                              NUM_JOINTS_HALF_BODY=njhb, PROB_HALF_BODY=PROB_HALF_BODY, COLOR_RGB=False),
                MODEL=types.SimpleNamespace(TARGET_TYPE="gaussian", IMAGE_SIZE=list(image_size), HEATMAP_SIZE=list(heatmap_size), SIGMA=SIGMA))
            ds = JointsDataset(cfg, "", "train", True, None)
            ds.num_joints, ds.flip_pairs, ds.upper_body_ids = J, pairs, upper_ids
            ds.aspect_ratio = image_size[0] * 1.0 / image_size[1]
            ds.db = [dict(image=name, annos=annos)]
            cand.append((si, name, njhb, ds, upper_ids))
    for seed in range(400):
        for si, name, njhb, ds, upper_ids in cand:
            if len(samples) >= MAX_SAMPLES or covered >= set(COVER):
                break
            rec = run_sample(ds, JointsDataset, seed, upper_ids)
            new = features(rec, name) - covered
            if new:
                covered |= new
                rec.update(set=si, njhb=njhb)
                samples.append(rec)
                print("seed %3d %-9s njhb %d: rot %8.3f sf %.4f half %d flip %d branches %s  (+ %s)"
                      % (seed, name, njhb, rec["rot"], rec["sf_ratio"], rec["half_flag"], rec["flip"], list(rec["half_body"]), sorted(new)))
    missing = set(COVER) - covered
    assert not missing, "not covered: %s" % sorted(missing)
    for a in annos:                                                    # __getitem__ works on a deep copy: the db is as it was
        assert a["center"].dtype == np.float32
    data["n_samples"] = np.int32(len(samples))
    for i, rec in enumerate(samples):
        for k, v in rec.items():
            data["s%d_%s" % (i, k)] = np.asarray(v)
    path = os.path.join(ROOT, "tests", "golden", "train_inputs_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(samples), "samples")


if __name__ == "__main__":
    main()
