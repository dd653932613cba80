"""-m gpu: the grouped forward with share_first_stage=True -- the models with a first stage of their own (TransPose-H, HRFormer; MODEL.NAME
interformer / interformer_2stage) run it once per person, hand over with one i2r_rows_gather_multi and run the tail per group -- at the
golden tags' own sizes with 2 to 9 persons.  Pinned to the reference through the existing goldens (whole-image groups: every person's map is
the ordinary forward's), and to the expanded forward of the same engine (share_first_stage=False, the path the project had before) on
proper sub-groups.  Bars: the project's fp32 bar (1e-3 max-abs) and bench.LP_TOL for the 16-bit modes.

Measured on MI355X (printed by the tests):
    whole-image groups vs the goldens, worst person: tph_l21 9.1e-6, hrt_l21 5.0e-5, hrt288_l2 3.7e-5, tph2s_l12 1.1e-5, ochtph_l21 1.2e-5,
        tph2s_dt_l12 1.6e-5, tph_up_l21 7.5e-5, tph2s_up_fk3_l12 8.8e-5, hrt_pre_nh2_l21 1.8e-4;
    [3, 1, 2] persons, shared vs expanded: 0 everywhere but max_patch 2 without the flip test: tph_l21 7.4e-6, tph2s_l12 9.3e-6
        (not bit-identical in general: the convs pick their tiles by the crop count; 1e-3 is asserted);  9 persons, capacity 10: 1.0e-5;
    bf16 tph_l21 9.41e-2 (1.49 % of max|ref|), fp16 hrt_l21 3.15e-2 (0.21 %): each equal to the ordinary forward's error."""
import numpy as np
import pytest
import torch

from i2r_amd import cabi, synth
from i2r_amd import input as i2r_input
from i2r_amd.engine import _multi
from test_main_target_gpu import FLIP_PAIRS, TOL, _expanded, _mt, _net

pytestmark = pytest.mark.gpu

_INPUTS = {}


def _inputs(length):
    key = tuple(length)
    if key not in _INPUTS:
        x, m, _ = synth.make_inputs(list(length), 256, 192)
        _INPUTS[key] = (x.cuda(), m.cuda())
    return _INPUTS[key]


def _boxes(n):
    b = _mt()[1]
    if n <= len(b):
        return b[:n].copy()
    u = synth.uniform01(3, "test_main_target_shared.boxes", 2 * n).reshape(n, 2)
    return u * [560.0, 400.0]


@pytest.mark.parametrize("tag", ["tph_l21", "hrt_l21", "hrt288_l2", "tph2s_l12", "ochtph_l21", "tph2s_dt_l12", "tph_up_l21", "tph2s_up_fk3_l12",
                                 "hrt_pre_nh2_l21"])
def test_whole_image_groups_match_the_existing_goldens(tag):
    """max_patch >= max(length): every group is its whole image with the target moved to the front, so every person's map must be the one
    the reference gave it.  tph2s_*: the third group's first member is crop 2 while its first row is row 3 -- a residual (or DOMAIN_TRANS
    input) taken from the wrong row misses the bar."""
    net, x, m, length, g = _net(tag)
    p = 3
    assert p >= max(length)
    boxes = _boxes(sum(length))
    if tag == "tph2s_l12":
        groups = i2r_input.main_target_groups(boxes, length, p)
        assert groups.group_len == [1, 2, 2] and groups.members.cpu().tolist() == [0, 1, 2, 2, 1]
    y = net.forward_main_target(x, m, length, boxes, max_patch=p, share_first_stage=True)
    torch.cuda.synchronize()
    err = np.abs(y.cpu().numpy() - g["out_multi"]).max(axis=(1, 2, 3))
    print("%s shared first stage, p=%d vs reference golden, per person max-abs %s" % (tag, p, ["%.2e" % e for e in err]))
    assert y.shape == g["out_multi"].shape and torch.isfinite(y).all() and (err < TOL).all(), err
    assert [k for P in net.engine().last_programs for k, _, _ in P.ops].count(cabi.GROUPS_OP_ROWS_GATHER_MULTI) == 2, "it really ran the shared program"


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("tag", ["tph_l21", "hrt_l21", "tph2s_l12"])
def test_sub_groups_against_the_expanded_forward(tag, p, flip):
    net = _net(tag)[0]
    length = [3, 1, 2]
    x, m = _inputs(length)
    boxes = _boxes(6)
    kw = dict(max_patch=p, flip_pairs=FLIP_PAIRS if flip else None)
    want = net.forward_main_target(x, m, length, boxes, share_first_stage=False, **kw).clone()
    got = net.forward_main_target(x, m, length, boxes, share_first_stage=True, **kw)
    torch.cuda.synchronize()
    err = (got - want).abs().max().item()
    print("%s shared vs expanded forward: max_patch %d flip %s max-abs %.3e" % (tag, p, flip, err))
    assert got.shape == want.shape == (6, net.cfg.MODEL.NUM_JOINTS, 64, 48) and torch.isfinite(got).all() and err < TOL, err


def test_capacity_slots_of_crops_groups_and_members():
    """9 persons: the program holds 10 crops, 18 members... and the stem, the position branch and the hand-over see only the 9 real ones"""
    net = _net("tph_l21")[0]
    eng = net.engine()
    length = [4, 5]
    x, m = _inputs(length)
    boxes = _boxes(9)
    want = net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=False).clone()
    got = net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=True)
    torch.cuda.synchronize()
    assert eng.capacity(9) == 10
    stem = [a for k, _, a in eng.last_programs[0].ops if k == cabi.OP_STEM and a.cin == 3]
    assert len(stem) == 1 and (stem[0].n_valid, stem[0].n_img) == (9, 10)
    err = (got - want).abs().max().item()
    print("9 persons in groups of 2, capacity 10: shared vs expanded forward max-abs %.3e" % err)
    assert got.shape == want.shape and err < TOL, err


@pytest.mark.parametrize("tag,precision", [("tph_l21", "bf16"), ("hrt_l21", "fp16")])
def test_16bit_modes_within_the_16bit_bar(tag, precision):
    import bench
    net, x, m, length, g = _net(tag, precision)
    ref = g["out_multi"]
    y = net.forward_main_target(x, m, length, _boxes(sum(length)), max_patch=3, share_first_stage=True)
    plain = _multi(net(x, m, length))
    torch.cuda.synchronize()
    err = np.abs(y.cpu().numpy() - ref).max()
    err_plain = np.abs(plain.cpu().numpy() - ref).max()
    print("%s %s vs fp32 reference golden: shared first stage max-abs %.3e = %.2f %% of max|ref|; ordinary forward %.3e"
          % (tag, precision, err, 100 * err / np.abs(ref).max(), err_plain))
    assert torch.isfinite(y).all() and err <= bench.LP_TOL[precision] * np.abs(ref).max()
    assert err > 1e-4  # it really is the 16-bit path


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("tag", ["tph_l21", "hrt_l21", "ochtph_l21"])
def test_first_stage_once_per_person_tail_once_per_group(tag, flip):
    net = _net(tag, "fp16" if tag == "hrt_l21" else "fp32")[0]  # (HRFormer: OP_HRT_ATTN is the attention half of the 16-bit modes' blocks)
    eng = net.engine()
    length = [3, 1, 2]
    x, m = _inputs(length)
    net.forward_main_target(x, m, length, _boxes(6), max_patch=2, flip_pairs=FLIP_PAIRS if flip else None, share_first_stage=True)
    torch.cuda.synchronize()
    S, G, N, k = 6, 11, 6, (2 if flip else 1)
    assert len(eng.last_programs) == 1, "one program"
    ops = eng.last_programs[0].ops
    stems = [a for kind, _, a in ops if kind == cabi.OP_STEM and a.cin == 3]
    assert len(stems) == 1 and stems[0].n_valid == S and stems[0].n_img == eng.capacity(S) * k, "the first stage saw S crops (and their mirrored copies)"
    enc = [a.n_tok for kind, _, a in ops if kind == cabi.OP_ENC_LAYER]
    inter = eng.capacity(G) * k * 16 * 12
    M = net.cfg.MODEL
    if tag == "hrt_l21":
        attn = [a.n_img for kind, _, a in ops if kind == cabi.OP_HRT_ATTN]
        assert attn and set(attn) == {eng.capacity(S) * k}, set(attn)
        win = [a.n_img for kind, _, a in ops if kind == cabi.OP_WINATTN]  # (the low-resolution branches keep the unfused form)
        assert set(win) <= {eng.capacity(S) * k}, set(win)
        assert enc and set(enc) == {inter}, set(enc)
    else:
        per_crop = eng.capacity(S) * k * eng.single_tokens
        assert per_crop != inter and set(enc) == {per_crop, inter}, set(enc)
        assert enc.index(inter) == enc.count(per_crop), "the per-crop layers come first"
    heads = [a for kind, _, a in ops if kind == cabi.OP_HEAD]
    assert len(heads) == 1 and heads[0].n_img == eng.capacity(N) * k, "no `single` head, the `multi` head once per group"
    kinds = [kind for kind, _, _ in ops]
    assert cabi.OP_ROWS_GATHER not in kinds, "no gather of the masks: the position branch runs on the distinct crops"
    assert kinds.count(cabi.GROUPS_OP_ROWS_GATHER_MULTI) == 2
    pos = [a for kind, _, a in ops if kind in (cabi.OP_STEM, cabi.OP_PE_RES_STEM) and getattr(a, "cin", 1) != 3]
    assert bool(pos) == bool(M.USE_MULTI_POS)
    if pos:  # (ochtph_l21: the `res` position branch)
        assert len(pos) == 1 and pos[0].n_valid == S and pos[0].n_img == eng.capacity(S) * k and pos[0].in_ == m.data_ptr()


def test_other_boxes_rebuild_nothing_and_change_the_affected_image_only():
    net = _net("tph_l21")[0]
    eng = net.engine()
    length = [2, 1, 3]
    x, m = _inputs(length)
    boxes = _boxes(6)
    a = net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=True).clone()
    n = eng.n_builds
    other = boxes.copy()
    other[4, :2] = (2000.0, 2000.0)  # person 1 of the last image moves far away: persons 0 and 2 of it become each other's neighbours
    b = net.forward_main_target(x, m, length, other, max_patch=2, share_first_stage=True).clone()
    torch.cuda.synchronize()
    g0, g1 = i2r_input.main_target_groups(boxes, length, 2), i2r_input.main_target_groups(other, length, 2)
    assert g0.group_len == g1.group_len and g0.members.cpu().tolist() != g1.members.cpu().tolist()
    assert eng.n_builds == n, "new boxes of the same sizes must not build a program"
    diff = (a - b).abs().amax(dim=(1, 2, 3)).cpu().numpy()
    print("per person max-abs change with other boxes:", ["%.2e" % d for d in diff])
    assert (diff[:3] == 0).all(), "images whose groups did not change give the same bits"
    assert (diff[3:] > 1e-4).any()
    assert torch.equal(net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=True), a), "back to the first boxes: the first result"


def test_defaults_are_unchanged():
    net = _net("tph_l21")[0]
    length = [3, 1, 2]
    x, m = _inputs(length)
    boxes = _boxes(6)
    off = net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=False).clone()
    assert torch.equal(net.forward_main_target(x, m, length, boxes, max_patch=2), off), "None on a TransPose-H model is the expanded forward"
    net, x, m, length, _ = _net("w48_l213")
    eng = net.engine()
    boxes = _mt()[1]
    net.forward_main_target(x, m, length, boxes, max_patch=2)
    *towers, tail = eng.last_programs
    assert towers and not any(kind in (cabi.OP_ENC_LAYER, cabi.OP_HEAD) for P in towers for kind, _, _ in P.ops), "None on the HRNet model still shares the tower"
    groups = i2r_input.main_target_groups(boxes, length, 2)
    want = _expanded(eng, x, m, groups)
    got = net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=False)
    torch.cuda.synchronize()
    assert torch.equal(got, want), "False on the HRNet model is the expanded forward"


@pytest.mark.parametrize("tag", ["ochtph_sine_l12", "tph_win_l12", "ochtph_cv_nh2_l21"])
def test_tails_that_cannot_take_gathered_rows_are_refused(tag):
    net, x, m, length, _ = _net(tag)
    boxes = _boxes(sum(length))
    with pytest.raises(ValueError, match="sine|window|cat_vec"):
        net.forward_main_target(x, m, length, boxes, max_patch=2, share_first_stage=True)
    y = net.forward_main_target(x, m, length, boxes, max_patch=2)  # None: expanded, as before
    torch.cuda.synchronize()
    assert y.shape[0] == sum(length) and torch.isfinite(y).all()
