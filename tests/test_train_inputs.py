"""Training samples, host side (i2r_amd.input: draw_augmentation, train_geometry and their parts) against
tests/golden/train_inputs_reference.npz, which the reference's own JointsDataset.__getitem__(is_train=True) wrote
(tools/make_golden_train_inputs.py; its pixel steps are oracle/input_cpu.py's restatement, not real cv2); the materialised pipeline of
tests/_train_input_ref.py against the fixture's crops and masks, bit for bit; and the C-ABI surface of i2r_train_inputs_cv2."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import _train_input_ref as tref
import _val_ref
from i2r_amd import cabi, caller
from i2r_amd import input as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = len(tref.fixture().samples)
PX_TOL = 1e-9   # px: both sides are float64 behind one 3x3 solve of the same well-conditioned point triples, coordinates < 2e3


def test_the_fixture_covers_every_branch_of_the_train_path():
    f = tref.fixture()
    S = f.samples
    rf, sf = f.rot_factor, f.scale_factor
    assert any(s.rot == 0 and s.rot_is_int for s in S) and any(s.rot != 0 for s in S)
    assert any(s.rot == -2 * rf for s in S) and any(s.rot == 2 * rf for s in S)
    assert any(s.sf_ratio == 1 - sf for s in S) and any(s.sf_ratio == 1 + sf for s in S)
    assert any(s.flip for s in S) and any(not s.flip for s in S)
    branches = set(int(b) for s in S for b in s.half_body)
    assert branches == {inp.HALF_BODY_OFF, inp.HALF_BODY_INELIGIBLE, inp.HALF_BODY_NONE, inp.HALF_BODY_UPPER, inp.HALF_BODY_LOWER}
    assert {s.joints.shape[1] for s in S} == {14, 17}
    for st in f.sets:   # a box sticking out of the image
        ih, iw = st.image.shape[:2]
        assert any(a["box"][0] + a["box"][2] > iw and a["box"][1] + a["box"][3] > ih for a in st.annos)
    assert f.sets[0].flip_pairs == caller.FLIP_PAIRS["coco"] and f.sets[1].flip_pairs == caller.FLIP_PAIRS["crowdpose"]
    assert f.sets[0].upper_body_ids == inp.UPPER_BODY_IDS["coco"] and f.sets[1].upper_body_ids == inp.UPPER_BODY_IDS["crowdpose"]
    assert os.path.getsize(tref.FIXTURE) < 400 * 1024


@pytest.mark.parametrize("i", range(N))
def test_draws_flip_branch_visibility_and_target_weight_are_the_references_exactly(i):
    f = tref.fixture()
    s = f.samples[i]
    (rot, sf_ratio, half_flag, flip), g, nxt = tref.replay(i)
    assert rot == s.rot and isinstance(rot, int) == s.rot_is_int and sf_ratio == s.sf_ratio
    assert half_flag is s.half_flag and flip is s.flip
    assert np.array_equal(g.half_body, s.half_body)
    assert np.array_equal(g.joints_vis, s.joints_vis)
    assert nxt == (float(s.next_py), float(s.next_np)), "both generators stand where the reference's __getitem__ left them"
    w, h = f.sets[s.set].heatmap_size
    _, tw = _val_ref.joint_targets(g.joints_hm[:, :, :2], g.joints_vis[:, :, 0], h, w, f.sigma)
    assert np.array_equal(tw, s.target_weight)
    assert (tw == 0).any() or (g.joints_vis[:, :, 0] > 0).all()


@pytest.mark.parametrize("i", range(N))
def test_centres_scales_and_joints_are_within_1e_9_px(i):
    s = tref.fixture().samples[i]
    _, g, _ = tref.replay(i)
    worst = {}
    for name, got, want, unit in (("center", g.center, s.center, 1.0), ("scale", g.scale, s.scale, 200.0), ("joints", g.joints, s.joints, 1.0),
                                  ("joints_hm", g.joints_hm, s.joints_hm, 1.0)):
        worst[name] = float(np.abs(got - want).max()) * unit
    print("sample %d (seed %d, rot %.3f, flip %d): max |diff| in px %s" % (i, s.seed, s.rot, s.flip, worst))
    assert all(v <= PX_TOL for v in worst.values()), worst
    # the formats too: a half-body scale is float32, a rescaled one float64 (numpy >= 2 promotion of the reference's s * sf_ratio)
    hb = np.isin(s.half_body, (inp.HALF_BODY_UPPER, inp.HALF_BODY_LOWER))
    assert np.array_equal(s.scale_is_f32, hb)
    assert np.array_equal(g.scale.astype(np.float32).astype(np.float64)[hb], g.scale[hb])


def test_generators_are_consumed_in_the_references_order():
    """draw_augmentation alone, against a replica that consumes in the order of JointsDataset.py:237-247: random() <= 0.6 first, randn()
    for the rotation only then, randn() for the scale, rand() for the half-body flag, random() for the flip only where flip is set"""
    seen = set()
    for seed in range(40):
        for flip in (True, False):
            py, npr = random.Random(seed), np.random.RandomState(seed)
            rot, sf_ratio, half_flag, flip_flag = inp.draw_augmentation(0.35, 45, flip, 0.3, np_random=npr, py_random=py)
            py2, np2 = random.Random(seed), np.random.RandomState(seed)
            rotated = py2.random() <= 0.6
            want_rot = np.clip(np2.randn() * 45, -90, 90) if rotated else 0
            want_sf = np.clip(np2.randn() * 0.35 + 1, 0.65, 1.35)
            want_half = np2.rand() < 0.3
            want_flip = flip and py2.random() <= 0.5
            assert (rot, sf_ratio, half_flag, flip_flag) == (want_rot, want_sf, want_half, want_flip)
            assert isinstance(rot, int) == (not rotated) and -90 <= rot <= 90 and 0.65 <= sf_ratio <= 1.35
            assert py.random() == py2.random() and npr.rand() == np2.rand()
            seen.add((rotated, flip))
    assert len(seen) == 4
    # the module-level generators are the default
    random.seed(5), np.random.seed(5)
    a = inp.draw_augmentation(0.35, 45, True, 0.3)
    assert a == inp.draw_augmentation(0.35, 45, True, 0.3, np_random=np.random.RandomState(5), py_random=random.Random(5))


def test_half_body_draws_its_coin_on_every_call_and_only_when_called():
    f = tref.fixture()
    st = f.sets[0]
    for half_flag, njhb, n_coins in ((False, 2, 0), (True, 8, 1), (True, 2, 3), (True, 99, 0)):
        npr = np.random.RandomState(3)
        g = inp.train_geometry(st.annos, (0, 1.0, half_flag, False), st.image.shape[:2], st.image_size, st.heatmap_size, st.flip_pairs,
                               st.upper_body_ids, num_joints_half_body=njhb, np_random=npr)
        ref = np.random.RandomState(3)
        for _ in range(n_coins):
            ref.randn()
        assert npr.rand() == ref.rand(), (half_flag, njhb)
        assert int((g.half_body >= inp.HALF_BODY_NONE).sum()) == n_coins
    for a in st.annos:   # nothing was modified (the fixture's arrays are read-only on top)
        assert a["center"].dtype == np.float32


@pytest.mark.parametrize("i", range(N))
def test_materialised_pipeline_reproduces_the_fixture_bit_for_bit(i):
    f = tref.fixture()
    s = f.samples[i]
    st = f.sets[s.set]
    _, g, _ = tref.replay(i)
    crops, masks = tref.materialised(st.image, g.trans, g.box, g.rotation, g.flip, st.image_size)
    assert crops.shape == s.crops.shape and masks.shape == s.masks.shape
    assert np.array_equal(crops, s.crops)
    assert np.array_equal(masks, s.masks)
    assert masks.max() == 255 and (s.rot == 0 or len(np.unique(masks)) > 2)
    M, nW, nH = inp.rotate_bound_geometry(st.image.shape[0], st.image.shape[1], g.rotation)
    assert (nW, nH) == g.canvas and tref.rotate_bound(np.zeros(st.image.shape[:2], np.uint8), g.rotation).shape == (nH, nW)


def test_train_affine_transform_keeps_the_references_float32_steps():
    """the reference's get_3rd_point runs in float32: the literal restatement differs from input.get_affine_transform (float64, rounded
    once) by up to an ulp of a float32 point coordinate -- visible, and far below a pixel"""
    rng = np.random.RandomState(0)
    worst = 0.0
    for k in range(200):
        c = np.array([rng.uniform(0, 130), rng.uniform(0, 97)], np.float32)
        s = np.array([rng.uniform(0.2, 1.0)] * 2, (np.float32, np.float64)[k % 2])
        r = (0, 30.0, -17.25, 80.0)[k % 4]
        a, b = inp.train_affine_transform(c, s, r, (48, 64)), inp.get_affine_transform(c, s, r, (48, 64))
        worst = max(worst, float(np.abs(a - b)[:, 2].max()))
        assert np.abs(a - b).max() < 1e-3
    assert worst > 1e-9


def test_batched_affine_transforms_take_a_rotation():
    rng = np.random.RandomState(1)
    cen = rng.uniform(0, 200, (30, 2)).astype(np.float32)
    scl = rng.uniform(0.2, 2.0, (30, 2)).astype(np.float32)
    rots = rng.uniform(-90, 90, 30)
    rots[::5] = 0
    for size in ((48, 64), (17, 23)):
        assert np.array_equal(inp.affine_transforms(cen, scl, size), np.stack([inp.get_affine_transform(cen[i], scl[i], 0, size) for i in range(30)]))
        assert np.array_equal(inp.affine_transforms(cen, scl, size, rot=0), inp.affine_transforms(cen, scl, size))
        per = np.stack([inp.get_affine_transform(cen[i], scl[i], rots[i], size) for i in range(30)])
        assert np.allclose(inp.affine_transforms(cen, scl, size, rot=rots), per, rtol=0, atol=1e-9)
        one = np.stack([inp.get_affine_transform(cen[i], scl[i], 30.0, size) for i in range(30)])
        assert np.allclose(inp.affine_transforms(cen, scl, size, rot=30.0), one, rtol=0, atol=1e-9)


def test_header_binding_exports_and_table_layout_agree_and_abi_stays_17(tmp_path):
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    assert re.search(r"^I2R_API\s+int\s+i2r_train_inputs_cv2\s*\(const i2r_image_ref\* images, int32_t n_images, const i2r_train_crop_ref\* crops, "
                     r"int32_t n_crops, int32_t swap_rb,\s*const float\* mean, const float\* inv_std, float\* x_out, float\* mask_out, int32_t oh, "
                     r"int32_t ow, void\* stream\);", header, flags=re.M)
    assert "i2r_train_inputs_cv2" in cabi.EXPORTS
    fields = ("inv_m", "mask_inv_m", "box", "nw", "nh", "image", "flip", "reserved")
    assert [n for n, _ in cabi.TrainCropRef._fields_] == list(fields) == list(inp._TRAIN_CROP_DT.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "i2r_hip.h"\nint main(void) { printf("%zu", sizeof(i2r_train_crop_ref));\n'
                   + "".join('printf(" %%zu", offsetof(i2r_train_crop_ref, %s));\n' % n for n in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    c_layout = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert c_layout[0] == 144 == ctypes.sizeof(cabi.TrainCropRef) == inp._TRAIN_CROP_DT.itemsize
    assert c_layout[1:] == [getattr(cabi.TrainCropRef, n).offset for n in fields] == [inp._TRAIN_CROP_DT.fields[n][1] for n in fields]
    assert c_layout[1:] == [0, 48, 96, 112, 116, 120, 124, 128]
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    assert "i2r_train_inputs_cv2" in __graft_entry__.exported_symbols(cabi.LIB_PATH)
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17 and L.i2r_train_inputs_cv2.argtypes is not None
