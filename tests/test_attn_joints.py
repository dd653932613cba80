"""CPU: the attention maps at the predicted joints (I2RModule.attention_at_joints) up to the device boundary -- the numpy restatement of
i2r_joint_tokens (tests/_attn_joints_ref.py: the literal get_max_preds, lib/core/inference.py:20-48) against the host path it replaces
(models/_base.points_to_tokens + group_tokens on 4 x arg-max), the C-ABI bookkeeping of the new entry, and JointForm.plan() against
literals worked by hand.  No GPU, no built library."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from _attn_joints_ref import crop_places, edge_maps, joint_tokens, max_preds
from i2r_amd import cabi
from i2r_amd.attn_capture import AttnQueries, JointForm, JointQueries, PersonMaps, QueryForm, resolve
from i2r_amd.models._base import group_tokens, points_to_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "i2r_hip.h")


# ---- the table rule ----
def test_edge_maps_hold_the_edges():
    hm = edge_maps(6, 17, 16, 12, 3)
    flat = hm.reshape(-1, 192)
    top = flat.max(1)
    assert any((row == m).sum() == 2 and m > 0 for row, m in zip(flat, top)), "no two-pixel tie"
    assert any(row.argmax() == 191 and m > 0 for row, m in zip(flat, top)), "no maximum at the last pixel"
    assert (top < 0).any() and any(not row.any() for row in flat), "no all-negative / all-zero map"


def test_restatement_follows_get_max_preds():
    hm = np.zeros((1, 4, 3, 5), dtype=np.float32)
    hm[0, 0, 1, 2] = hm[0, 0, 2, 4] = 0.5    # a tie: the first index wins
    hm[0, 1, 2, 4] = 0.25                    # the last pixel
    hm[0, 2] = -1.0                          # nothing positive: pred_mask zeroes the point, the maximum is reported as it is
    preds, maxvals = max_preds(hm)           # (map 3 is all zero)
    assert preds.tolist() == [[[2.0, 1.0], [4.0, 2.0], [0.0, 0.0], [0.0, 0.0]]] and maxvals.tolist() == [[0.5, 0.25, -1.0, 0.0]]
    tab = dict(n_grp=1, K=4, fh=2, fw=3, down=8, group=[0], slot=[0])
    points, _, (tok,) = joint_tokens(hm, 4, [tab])
    # (x, y) = (8, 4) -> (row 0, col 1); (16, 8) -> (row 1, col 2); the masked maps -> the token of (0, 0), not a skip
    assert points.tolist() == [[[8.0, 4.0], [16.0, 8.0], [0.0, 0.0], [0.0, 0.0]]] and tok.tolist() == [[1, 5, 0, 0]]
    # the clamp: an 8 x 8 map at stride 4 on a 1 x 1 token map of down rate 16
    hm = np.zeros((1, 1, 8, 8), dtype=np.float32)
    hm[0, 0, 7, 7] = 1.0
    assert joint_tokens(hm, 4, [dict(n_grp=1, K=1, fh=1, fw=1, down=16, group=[0], slot=[0])])[2][0].tolist() == [[0]]


@pytest.mark.parametrize("length,hh,hw,fh,fw,down", [([1, 3, 2], 16, 12, 4, 3, 16), ([2, 1], 64, 48, 16, 12, 16), ([1, 1, 4], 64, 48, 64, 48, 4),
                                                     ([3], 5, 3, 5, 3, 4)])
def test_restatement_equals_the_host_path(length, hh, hw, fh, fw, down):
    """the tables the device makes = group_tokens(points_to_tokens(4 * argmax, ...)) of the host path, for both kinds of stack"""
    S, J = sum(length), 17
    hm = edge_maps(S, J, hh, hw, 7 * hh + S)
    idx = torch.from_numpy(hm).reshape(S, J, -1).argmax(-1)
    idx = torch.where(torch.from_numpy(hm).reshape(S, J, -1).amax(-1) > 0, idx, torch.zeros_like(idx))  # pred_mask
    pts = 4 * torch.stack([idx % hw, idx // hw], -1)
    tok = points_to_tokens(pts, 4 * hh, 4 * hw, fh, fw)
    assert 4 * hh // fh == down
    tabs = []
    for intra in (True, False):
        group, slot = crop_places(length, intra)
        tabs.append(dict(n_grp=S if intra else len(length), K=J if intra else max(length) * J, fh=fh, fw=fw, down=down, group=group, slot=slot))
    points, maxvals, (t_intra, t_inter) = joint_tokens(hm, 4, tabs)
    assert np.array_equal(points, pts.numpy().astype(np.float32)) and np.array_equal(maxvals, hm.reshape(S, J, -1).max(-1))
    assert np.array_equal(t_intra, tok.numpy())
    want, counts = group_tokens(tok, length, fh * fw)
    assert np.array_equal(t_inter, want.numpy()) and counts == [n * J for n in length]
    assert (t_inter == -1).sum() == sum((max(length) - n) * J for n in length)


# ---- the C-ABI ----
def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = [re.sub(r"\[.*\]", "", n.strip().lstrip("*").strip()) for n in decl.split(",")]
        names[0] = re.sub(r"\[.*\]", "", names[0].split()[-1].lstrip("*"))
        out += names
    return out


def test_header_and_ctypes_agree():
    text = open(HEADER).read()
    assert re.search(r"^I2R_API int i2r_joint_tokens\(const i2r_joint_tokens_args\* a, void\* stream\);", text, flags=re.M)
    assert "i2r_joint_tokens" in cabi.EXPORTS
    assert "#define I2R_ABI_VERSION 17\n" in text and cabi.ABI_VERSION == 17, "the new entry is additive"
    assert "#define I2R_MAX_TOKEN_TABLES 2\n" in text and cabi.MAX_TOKEN_TABLES == 2
    assert [n for n, _ in cabi.TokenTable._fields_] == _struct_fields(text, "i2r_token_table")
    assert [n for n, _ in cabi.JointTokensArgs._fields_] == _struct_fields(text, "i2r_joint_tokens_args")
    # three pointers + six int32; three pointers + two tables + six int32: no padding anywhere
    assert ctypes.sizeof(cabi.TokenTable) == 48 and ctypes.sizeof(cabi.JointTokensArgs) == 24 + 2 * 48 + 24
    assert cabi.JointTokensArgs.table.offset == 24 and cabi.JointTokensArgs.n_crops.offset == 120


# ---- the plan ----
INTER, INTRA = "enc", "singleformer.enc"
CAP = frozenset({(INTER, 0), (INTRA, 1)})


def check_plan_literals():
    """length [1, 3, 2], J = 17, an inter-human stack of 4 x 3 tokens (groups = images) and an intra-human stack of 16 x 12 (groups = crops)"""
    f = JointForm(CAP, JointQueries("dependency", {INTER: 2, INTRA: 4}), 17)
    assert f.deferred and not QueryForm.deferred and f.J == 17 and f.mode == 0
    p = f.plan(INTER, (4, 3), [12, 36, 24], 2, f.call)
    assert (p.n_grp, p.K, p.ws_stride, p.ws_floats, p.rows_floats) == (3, 51, 4, 612, 3672)
    assert (p.blocks[0].offs, p.layer_floats, p.n_tiles, p.n_col_tiles) == ([0, 816, 8160, 11424], 11424, 9, 0)
    assert p.blocks[0].shapes == [(17, 1, 8, 6), (51, 3, 8, 6), (34, 2, 8, 6)]
    shape, cnt, crops = p.tables
    assert shape == (3, 51) and cnt.tolist() == [17, 51, 34] and cnt.dtype == torch.int32
    assert crops.tolist() == [[0, 1, 1, 1, 2, 2], [0, 0, 1, 2, 0, 1]] and crops.dtype == torch.int32 and crops.is_contiguous()
    p = f.plan(INTRA, (16, 12), [192] * 6, 2, f.call)
    assert (p.n_grp, p.K, p.ws_stride, p.ws_floats, p.rows_floats, p.layer_floats, p.n_tiles) == (6, 17, 8, 816, 19584, 313344, 24)
    assert p.blocks[0].offs[:3] == [0, 52224, 104448] and p.blocks[0].shapes == [(17, 1, 64, 48)] * 6
    assert p.tables[0] == (6, 17) and p.tables[1].tolist() == [17] * 6 and p.tables[2].tolist() == [[0, 1, 2, 3, 4, 5], [0] * 6]
    g = JointForm(CAP, JointQueries("affect", 1), 17)
    p = g.plan(INTER, (4, 3), [12, 36, 24], 2, g.call)
    assert (p.ws_floats, p.rows_floats, p.n_tiles, p.n_col_tiles, p.layer_floats) == (288, 1, 6, 20, 2856)
    # the same layout as the query form asked with the tables the device will make
    q = AttnQueries({INTER: torch.zeros(3, 51, dtype=torch.int32)}, "affect", 1, {INTER: [17, 51, 34]}, capacity=17)
    w = QueryForm(frozenset({(INTER, 0)}), q).plan(INTER, (4, 3), [12, 36, 24], 2, q)
    assert (w.ws_stride, w.ws_floats, w.rows_floats, w.blocks, w.layer_floats, w.n_tiles, w.n_col_tiles, w.K) == \
        (p.ws_stride, p.ws_floats, p.rows_floats, p.blocks, p.layer_floats, p.n_tiles, p.n_col_tiles, p.K)


def check_forms():
    stacks = {INTRA: 4, INTER: 6}
    args = (stacks, INTER, False)
    j = JointQueries("affect", {INTER: 16, INTRA: 4})
    for flip in (None, "flip"):  # the one form that goes with the flip test
        f = resolve(CAP, None, None, flip, *args, joints=j, n_joints=17)
        assert type(f) is JointForm and f.call is j
        assert f.key == ("capture", CAP, "query", 1, 17, ((INTER, 16), (INTRA, 4)), "joints")
    q = AttnQueries({INTER: torch.zeros(2, 17), INTRA: torch.zeros(4, 17)}, "affect", {INTER: 16, INTRA: 4}, capacity=17)
    assert resolve(CAP, q, None, None, *args).key == f.key[:-1], "the marker is all that tells the two programs apart"
    for kw, window, st, match in ((dict(queries=q), False, stacks, "not with"), (dict(persons=PersonMaps()), False, stacks, "not with"),
                                  ({}, True, stacks, "ATTENTION_TYPE window"), ({}, False, {}, "no encoder stack")):
        with pytest.raises(ValueError, match=match):
            resolve(CAP, kw.get("queries"), kw.get("persons"), None, st, INTER, window, joints=j, n_joints=17)
    with pytest.raises(ValueError, match="needs capture"):
        resolve((), None, None, None, *args, joints=j, n_joints=17)
    with pytest.raises(ValueError, match="encoder stacks are"):
        resolve({(INTER, 6)}, None, None, None, *args, joints=j, n_joints=17)
    with pytest.raises(ValueError, match="upsample"):
        resolve(CAP, None, None, None, *args, joints=JointQueries(upsample=65), n_joints=17)
    with pytest.raises(ValueError, match="mode"):
        JointQueries("both")
    # the refusals of the other forms with the flip test stay
    with pytest.raises(ValueError, match="not with"):
        resolve({(INTER, 0)}, None, PersonMaps(), "flip", *args)
    with pytest.raises(AssertionError):
        resolve(CAP, None, None, "flip", *args)
    with pytest.raises(AssertionError):
        resolve(CAP, q, None, "flip", *args)


def check_all():
    check_plan_literals()
    check_forms()


def test_plan_literals():
    check_plan_literals()


def test_form_key_and_refusals():
    check_forms()


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import torch
import i2r_amd
from i2r_amd import cabi
def touched(*a, **k):
    raise RuntimeError("the planner touched the device or the library")
cabi.lib = cabi.load_library = torch.cuda._lazy_init = torch.cuda.init = touched
import test_attn_joints
test_attn_joints.check_all()
assert cabi._LIB is None and not torch.cuda.is_initialized() and "i2r_amd.engine" not in sys.modules
print("planned in isolation")
"""


def test_planning_needs_no_device_and_no_library():
    """the plan cases first thing in a fresh interpreter in which loading the library or initialising the device raises"""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "planned in isolation" in r.stdout, r.stdout + r.stderr
