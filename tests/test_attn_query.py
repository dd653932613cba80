"""CPU: the surface of the attention maps at query points -- the C-ABI declaration of i2r_attn_query_maps and its op kind, the point ->
token mapping of net.attention_at, and the float64 helper (tests/_attn_query_ref.py) against the reference's own hook rows."""
import os
import re

import numpy as np
import pytest
import torch

from _attn_query_ref import point_of_token, query_maps
from _attn_ref import restate
from _golden import GOLDEN, setup
from i2r_amd import cabi
from i2r_amd.models._base import group_tokens, points_to_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["w48_l31", "tph_l21", "w48_nh8_l21", "hrt_pre_nh2_l21"]


def test_header_declares_attn_query_maps_and_op_kind():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert re.search(r"^I2R_API int i2r_attn_query_maps\(const i2r_attn_query_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"I2R_OP_ATTN_QUERY = 30\b", header) and cabi.CAPTURE_OP_ATTN_QUERY == 30
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == cabi.ABI_VERSION == 17
    assert "i2r_attn_query_maps" in cabi.EXPORTS
    fields = re.search(r"typedef struct i2r_attn_query_args \{(.*?)\} i2r_attn_query_args;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in cabi.AttnQueryArgs._fields_]
    n_ptr = sum(1 for _, t in cabi.AttnQueryArgs._fields_ if t is cabi._fp)
    assert n_ptr == 9 and names[:n_ptr] == [f for f, t in cabi.AttnQueryArgs._fields_ if t is cabi._fp]  # pointers first: no padding holes
    api = open(os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc", "i2r_api.hip")).read()
    assert re.search(r"case I2R_OP_ATTN_QUERY: rc = i2r_attn_query_maps\(", api)  # (one runner serves i2r_run_program and _timed)


def test_points_to_tokens_edges():
    H, W, fh, fw = 256, 192, 64, 48  # down_rate 4
    pts = torch.tensor([[[0.0, 0.0], [W - 1, 0.0], [0.0, H - 1], [W - 1, H - 1], [3.999, 4.0], [float("nan"), 5.0], [7.0, float("nan")]]])
    tok = points_to_tokens(pts, H, W, fh, fw)
    assert tok.dtype == torch.int32 and tok.shape == (1, 7)
    assert tok[0].tolist() == [0, fw - 1, (fh - 1) * fw, fh * fw - 1, 1 * fw + 0, -1, -1]
    # the inter-human token map of the same input: 16 x 12, down_rate 16 (= input height // feature height, visualize.py:194-196)
    assert points_to_tokens(torch.tensor([[[191.0, 255.0], [16.0, 15.9]]]), H, W, 16, 12)[0].tolist() == [16 * 12 - 1, 1]
    # a numpy array of doubles works as well
    assert points_to_tokens(np.array([[[4.0, 8.0]]]), H, W, fh, fw)[0].tolist() == [2 * fw + 1]


@pytest.mark.parametrize("pt", [[-0.5, 3.0], [192.0, 3.0], [3.0, 256.0], [3.0, -1e-3], [float("inf"), 0.0]])
def test_point_outside_the_crop_raises(pt):
    with pytest.raises(ValueError):
        points_to_tokens(torch.tensor([[[1.0, 1.0], pt]]), 256, 192, 64, 48)


def test_points_shape_is_checked():
    with pytest.raises(ValueError):
        points_to_tokens(torch.zeros(3, 2), 256, 192, 64, 48)


def test_multi_person_token_layout():
    """inter-human stack: the group is the image, entry person * K + k holds token person * hw + (y, x); padding and skipped points stay -1"""
    hw, K = 192, 3
    tok = torch.tensor([[0, 5, -1], [191, 7, 7], [1, 2, 3], [4, -1, 6], [10, 11, 12], [13, 14, 15]], dtype=torch.int32)
    table, counts = group_tokens(tok, [2, 1, 3], hw)
    assert table.dtype == torch.int32 and table.shape == (3, 9) and counts == [6, 3, 9]
    assert table[0].tolist() == [0, 5, -1, hw + 191, hw + 7, hw + 7, -1, -1, -1]
    assert table[1].tolist() == [1, 2, 3] + [-1] * 6
    assert table[2].tolist() == [4, -1, 6, hw + 10, hw + 11, hw + 12, 2 * hw + 13, 2 * hw + 14, 2 * hw + 15]


def test_point_of_token_round_trips():
    toks = [0, 47, 48, 64 * 48 - 1, 1234]
    pts = torch.tensor([[point_of_token(t, 48, 4) for t in toks]])
    assert points_to_tokens(pts, 256, 192, 64, 48)[0].tolist() == toks


def test_helper_rows_columns_and_interpolate():
    g = torch.Generator().manual_seed(3)
    P, h, w = 2, 3, 4
    full = torch.rand(P * h * w, P * h * w, generator=g, dtype=torch.float64)
    toks = [0, 23, 5, 5, -1]
    r = query_maps(full, toks, 0, h, w)
    c = query_maps(full, toks, 1, h, w)
    assert r.shape == c.shape == (5, P, h, w)
    assert torch.equal(r[1].reshape(-1), full[23]) and torch.equal(c[2].reshape(-1), full[:, 5]) and torch.equal(r[2], r[3])
    assert not r[4].any() and not c[4].any()
    up = query_maps(full, toks, 0, h, w, 3)
    assert up.shape == (5, P, 9, 12) and up.dtype == torch.float64
    # align_corners=False with an integer scale: source coordinate (dst + 0.5) / scale - 0.5, clamped at 0, neighbours clamped at the edge
    m = r[1, 1]
    for oy, ox in [(0, 0), (4, 7), (8, 11), (1, 10)]:
        sy, sx = max((oy + 0.5) / 3 - 0.5, 0.0), max((ox + 0.5) / 3 - 0.5, 0.0)
        y0, x0 = int(sy), int(sx)
        y1, x1, ly, lx = min(y0 + 1, h - 1), min(x0 + 1, w - 1), sy - int(sy), sx - int(sx)
        want = (1 - ly) * ((1 - lx) * m[y0, x0] + lx * m[y0, x1]) + ly * ((1 - lx) * m[y1, x0] + lx * m[y1, x1])
        assert abs(up[1, 1, oy, ox].item() - want.item()) < 1e-12


@pytest.mark.parametrize("tag", FIXTURES)
def test_helper_on_restatement_reproduces_reference_hook_rows(tag):
    """mode 0 with the fixture's `rows` as query tokens == the reference's own hook rows within the restatement's 2e-5"""
    cfg, sd, x, m, length, _ = setup(tag)
    fx = dict(np.load(os.path.join(GOLDEN, "attn_%s.npz" % tag)))
    maps, feats, _ = restate(cfg, sd, x, m, length)
    seen = 0
    for (st, l), w in maps.items():
        h, wd = feats[st].shape[2:]
        for b, n in enumerate(int(v) for v in fx["%s.lens" % st]):
            rows = fx["%s.%d.%d.rows" % (st, l, b)]
            assert rows.max() < n
            got = query_maps(w[b, :n, :n], rows, 0, h, wd).reshape(len(rows), n)
            err = np.abs(got.numpy() - fx["%s.%d.%d.maps" % (st, l, b)][:, :n]).max()
            assert err < 2e-5, "%s %s.%d entry %d: max-abs %.2e" % (tag, st, l, b, err)
            seen += 1
    assert seen == sum(1 for k in fx if k.endswith(".maps"))
