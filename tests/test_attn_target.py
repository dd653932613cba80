"""CPU: the surface of the target form of the attention per person (grouped inference) -- the C-ABI declaration of i2r_attn_target_maps
and its op kind, TargetForm.plan() against a restatement of the header comment, and every refusal of attn_capture.resolve and
net.main_target_relations that needs no engine."""
import ctypes
import os
import re

import pytest
import torch

from i2r_amd import attn_capture, cabi, config, models
from i2r_amd.engine import Engine, TargetMaps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST = "global_encoder"
STACKS = {"singleformer.global_encoder": 4, ST: 2}


def test_header_declares_attn_target_maps_and_op_kind():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert re.search(r"^I2R_API int i2r_attn_target_maps\(const i2r_attn_target_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"I2R_OP_ATTN_TARGET = 33\b", header) and cabi.CAPTURE_OP_ATTN_TARGET == 33
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == cabi.ABI_VERSION == 17  # additive: unchanged
    assert "i2r_attn_target_maps" in cabi.EXPORTS
    fields = re.search(r"typedef struct i2r_attn_target_args \{(.*?)\} i2r_attn_target_args;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in cabi.AttnTargetArgs._fields_]
    n_ptr = sum(1 for _, t in cabi.AttnTargetArgs._fields_ if t is cabi._fp)
    assert n_ptr == 9 and names[:n_ptr] == [f for f, t in cabi.AttnTargetArgs._fields_ if t is cabi._fp]  # pointers first: no padding holes
    assert all(t is cabi._i32 for _, t in cabi.AttnTargetArgs._fields_[n_ptr:])
    assert ctypes.sizeof(cabi.AttnTargetArgs) == 8 * n_ptr + 4 * (len(names) - n_ptr) == 120
    api = open(os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc", "i2r_api.hip")).read()
    assert re.search(r"case I2R_OP_ATTN_TARGET: rc = i2r_attn_target_maps\(", api)


def test_built_library_exports_attn_target_maps():
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert L.i2r_attn_target_maps.argtypes[0]._type_ is cabi.AttnTargetArgs
    assert L.i2r_attn_target_maps(None, None) == -1 and b"null pointer" in L.i2r_last_error()  # (rejected on the host: no GPU needed)


def _up4(n):
    return -(-n // 4) * 4


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("mode,kind", [(0, None), (1, "dependency"), (2, "affect")])
@pytest.mark.parametrize("heads", [1, 8])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 1), (8, 6), (16, 12)])
@pytest.mark.parametrize("members", [[1], [2, 1], [3, 6, 1, 2]])
def test_plan_is_the_headers_layout(members, h, w, heads, mode, kind, scale):
    """include/i2r_hip.h, i2r_attn_target_maps: ws = ws_stride floats per token row, ws_stride >= 2 heads ceil(max L_g / 128); rows =
    grp_off[n_grp] floats, twice that for mode 1 at scale > 1; rel block of group g = m_g floats, maps block = L_g scale^2 floats
    = [m_g, h scale, w scale]; here group g's blocks lie g * slots entries into their set, every set on a 16-byte boundary"""
    seg = h * w
    lens = [m * seg for m in members]
    for slots in (None, max(members), max(members) + 2):
        req = TargetMaps(kind, scale, slots=slots)
        form = attn_capture.resolve({(ST, 1)}, None, None, None, STACKS, ST, False, targets=req)
        assert isinstance(form, attn_capture.TargetForm) and isinstance(form, attn_capture.Form)
        assert form.key == ("capture", frozenset({(ST, 1)}), "targets", mode, scale) and form.call is req and not form.deferred
        p = form.plan(ST, (h, w), lens, heads, req)
        width = slots or max(members)
        ints = [p.n_grp, p.ws_stride, p.ws_floats, p.rows_floats, p.layer_floats, p.K] + [b.base for b in p.blocks] + [o for b in p.blocks for o in b.offs]
        assert all(type(v) is int for v in ints), "a plan holds nothing but integers"
        assert p.tables == () and p.extra_floats == 0 and p.raw_floats == 0
        assert p.n_grp == len(members) and p.K == width
        assert p.ws_stride == 2 * heads * -(-max(lens) // 128) and p.ws_floats == p.ws_stride * sum(lens)
        assert p.rows_floats == (2 if mode == 1 and scale > 1 else 1) * sum(lens)
        rel, maps = p.blocks
        assert rel.base == 0 and rel.offs == [g * width for g in range(len(members) + 1)] and rel.shapes == [(m,) for m in members]
        assert maps.base == _up4(len(members) * width) and maps.base % 4 == 0
        per = h * scale * w * scale
        if mode:
            assert maps.offs == [g * width * per for g in range(len(members) + 1)]
            assert maps.shapes == [(m, h * scale, w * scale) for m in members]
            assert p.layer_floats == maps.base + _up4(len(members) * width * per)
            assert all(m * per == n * scale * scale for m, n in zip(members, lens))  # the header's L_g scale^2 floats
        else:
            assert maps.shapes is None and not any(maps.offs) and p.layer_floats == maps.base
        assert p.layer_floats % 4 == 0
    with pytest.raises(ValueError, match="members"):
        form.plan(ST, (h, w), [n + seg for n in lens], heads, TargetMaps(kind, scale, slots=max(members)))


def test_patch_fills_the_per_call_fields():
    form = attn_capture.TargetForm(frozenset({(ST, 0)}), TargetMaps("affect", 2))
    p = form.plan(ST, (4, 3), [36, 12], 8, form.call)
    a = cabi.AttnTargetArgs()
    form.patch(a, p, 4096, 64, 128, [], 256)
    assert (a.rel, a.maps, a.ws, a.rows, a.grp_off_host, a.n_grp, a.ws_stride) == (4096, 4096 + 4 * p.blocks[1].base, 64, 128, 256, 2, 16)


def test_target_maps_request():
    assert (TargetMaps().mode, TargetMaps("dependency").mode, TargetMaps("affect", 4).mode, TargetMaps("affect", 4).scale) == (0, 1, 2, 4)
    assert TargetMaps().slots is None and TargetMaps(slots=3).slots == 3
    for bad in ("rows", 3, True, 1):
        with pytest.raises(ValueError, match="maps"):
            TargetMaps(bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="scale"):
            TargetMaps("affect", bad)
    with pytest.raises(ValueError, match="slots"):
        TargetMaps(slots=0)


def test_resolve_refuses_what_the_target_form_does_not_serve():
    t, cap = TargetMaps("dependency"), {(ST, 0)}
    ok = attn_capture.resolve(cap, None, None, None, STACKS, ST, False, targets=t)
    assert isinstance(ok, attn_capture.TargetForm)
    jm = torch.zeros(17, dtype=torch.int32)
    for kw, msg in ((dict(persons=attn_capture.PersonMaps()), "not with"), (dict(rollout=attn_capture.Rollout(None, None)), "not with"),
                    (dict(queries=attn_capture.AttnQueries({ST: torch.zeros(1, 1, dtype=torch.int32)})), "not with"),
                    (dict(joints=attn_capture.JointQueries()), "not with"),
                    (dict(flip_joint_map=jm), "flip test"), (dict(flip_maps="merged", flip_joint_map=jm), "flip test"),
                    (dict(window=True), "window"), (dict(capture=None), "needs capture"), (dict(capture=set()), "needs capture"),
                    (dict(capture={("singleformer.global_encoder", 0)}), "inter-human stack"),
                    (dict(capture={(ST, 0), ("singleformer.global_encoder", 1)}), "inter-human stack"),
                    (dict(capture={(ST, 2)}), "encoder stacks"), (dict(capture={(ST, -1)}), "encoder stacks"),
                    (dict(stacks={"singleformer.global_encoder": 4}), "inter-human stack"), (dict(targets=object()), "TargetMaps")):
        d = dict(capture=cap, queries=None, persons=None, flip_joint_map=None, stacks=STACKS, inter_stack=ST, window=False, targets=t)
        d.update(kw)
        with pytest.raises(ValueError, match=msg):
            attn_capture.resolve(**d)


class _Stub:
    """what Engine.forward_groups reads before it resolves the form"""
    inter_stack, window_attn = ST, False

    @staticmethod
    def capture_stacks():
        return dict(STACKS)


def test_forward_groups_refuses_before_anything_touches_a_device():
    x, m, mem = torch.zeros(1, 3, 256, 192), torch.zeros(1, 1, 256, 192), torch.zeros(1, dtype=torch.int32)
    t = TargetMaps()
    with pytest.raises(ValueError, match="persons= is not served"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], persons=object(), relations=t, capture={(ST, 0)})
    with pytest.raises(ValueError, match="rollout= is not served"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], rollout=object(), relations=t, capture={(ST, 0)})
    with pytest.raises(ValueError, match="flip test"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], flip_joint_map=torch.zeros(17, dtype=torch.int32), relations=t, capture={(ST, 0)})
    with pytest.raises(ValueError, match="inter-human stack"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], relations=t, capture={("singleformer.global_encoder", 0)})
    with pytest.raises(ValueError, match="needs capture"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], relations=t)
    with pytest.raises(ValueError, match="goes with relations"):
        Engine.forward_groups(_Stub(), x, m, mem, [1], capture={(ST, 0)})
    win = _Stub()
    win.window_attn = True
    with pytest.raises(ValueError, match="window"):
        Engine.forward_groups(win, x, m, mem, [1], relations=t, capture={(ST, 0)})


def test_main_target_relations_raises_without_an_engine():
    x, m, boxes = torch.zeros(1, 3, 256, 192), torch.zeros(1, 1, 256, 192), torch.zeros(1, 4, dtype=torch.float64)
    cfg = config.load_config("tph_192_p6_b4")
    with pytest.raises(ValueError, match="no inter-human stack"):
        models.transpose_h.get_pose_net(cfg, is_train=False).main_target_relations(x, m, [1], boxes, max_patch=2)
    with pytest.raises(ValueError, match="no inter-human stack"):
        models.hrformer.get_pose_net(config.load_config("hrt_192_p4_b4"), is_train=False).main_target_relations(x, m, [1], boxes, max_patch=2)
    win = config.load_config("tph_192_p6_b4", ["MODEL.ATTENTION_TYPE", "window", "MODEL.N_HEAD", 4])
    with pytest.raises(ValueError, match="ATTENTION_TYPE"):
        models.interformer.get_pose_net(win, is_train=False).main_target_relations(x, m, [1], boxes, max_patch=2)
    net = models.interformer.get_pose_net(cfg, is_train=False)
    for bad in ("rows", True, 2):
        with pytest.raises(ValueError, match="maps"):
            net.main_target_relations(x, m, [1], boxes, max_patch=2, maps=bad)
    with pytest.raises(ValueError, match="flip_pairs"):
        net.main_target_relations(x, m, [1], boxes, max_patch=2, flip_pairs=[[1, 2]])
    # the refusals that predate this method stay as they are
    with pytest.raises(ValueError, match="rollout= is not served"):
        net.forward_main_target(x, m, [1], boxes, max_patch=2, rollout=object())
