"""-m gpu: the attention maps at the predicted joints on the MI355X -- the raw i2r_joint_tokens C-ABI bit for bit against the numpy
restatement of get_max_preds and the table rule (tests/_attn_joints_ref.py) on poisoned, canary-guarded buffers; net.attention_at_joints
against the two-call flow it replaces (forward, arg-max on the host, attention_at), plain and under the flip test; program reuse,
non-interference and the refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from _attn_joints_ref import crop_places, edge_maps, joint_tokens
from _golden import keys_manifest, setup
from i2r_amd import caller, cabi, config, models, synth
from i2r_amd.engine import AttnQueries, JointQueries, PersonMaps

pytestmark = pytest.mark.gpu
PAD = 7  # canary words in front of and behind every buffer (odd: the buffers themselves are only 4-byte aligned)
F_CANARY, F_POISON = 12345.0, -7777.0
I_CANARY, I_POISON = 0x5A5A5A5A, 0x3C3C3C3C


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dtype):
    """a poisoned buffer between two rows of canary words -> (whole allocation, the buffer's view)"""
    n = int(np.prod(shape))
    canary, poison = (F_CANARY, F_POISON) if dtype == torch.float32 else (I_CANARY, I_POISON)
    whole = torch.full((n + 2 * PAD,), canary, dtype=dtype, device="cuda")
    whole[PAD:PAD + n] = poison
    return whole, whole[PAD:PAD + n].view(shape)


def _canaries_intact(whole):
    canary = F_CANARY if whole.dtype == torch.float32 else I_CANARY
    return bool((whole[:PAD] == canary).all()) and bool((whole[-PAD:] == canary).all())


def _tables(length, specs):
    """specs: (intra, n_grp, K, fh, fw, down) -> the restatement's table dicts"""
    out = []
    for intra, n_grp, K, fh, fw, down in specs:
        group, slot = crop_places(length, intra)
        out.append(dict(n_grp=n_grp, K=K, fh=fh, fw=fw, down=down, group=group, slot=slot))
    return out


def _args(hm, points, maxvals, tabs, dev, in_stride=4, **over):
    S, J, hh, hw = hm.shape
    a = cabi.JointTokensArgs(heatmaps=hm.data_ptr(), points=points.data_ptr() if points is not None else None,
                             maxvals=maxvals.data_ptr() if maxvals is not None else None, n_crops=S, joints=J, hh=hh, hw=hw, in_stride=in_stride,
                             n_tables=len(tabs))
    for t, spec, (tok, grp, slot) in zip(a.table, tabs, dev):
        t.tokens, t.crop_group, t.crop_slot = tok.data_ptr(), grp.data_ptr(), slot.data_ptr()
        t.n_grp, t.K, t.fh, t.fw, t.down = spec["n_grp"], spec["K"], spec["fh"], spec["fw"], spec["down"]
    for k, v in over.items():
        if k.startswith("t0_"):
            setattr(a.table[0], k[3:], v)
        else:
            setattr(a, k, v)
    return a


# (n_crops, J, hh, hw), length, tables (intra, n_grp, K, fh, fw, down)
RAW = {
    "1x1x1x1": ((1, 1, 1, 1), [1], [(True, 1, 1, 1, 1, 4)]),
    "3x14x5x3-short-of-a-wave": ((3, 14, 5, 3), [3], [(True, 3, 14, 5, 3, 4)]),
    "6x17x16x12-images-1-3-2": ((6, 17, 16, 12), [1, 3, 2], [(False, 3, 51, 4, 3, 16)]),
    # two tables in one call; the first with a row stride beyond its entries and a group no crop belongs to
    "2x17x64x48-two-tables": ((2, 17, 64, 48), [2], [(False, 2, 40, 16, 12, 16), (True, 2, 17, 64, 48, 4)]),
}


@pytest.mark.parametrize("case", sorted(RAW))
def test_raw_tokens_points_maxvals_match_the_restatement_bitwise(case):
    (S, J, hh, hw), length, specs = RAW[case]
    hm = edge_maps(S, J, hh, hw, 11 * S + hh)
    if S * J >= 5:  # the edges are in: a first-wins tie, the last pixel, an all-negative and an all-zero map
        flat = hm.reshape(S * J, -1)
        assert any((r == r.max()).sum() == 2 for r in flat) and any(r.argmax() == hh * hw - 1 for r in flat)
        assert (flat.max(1) < 0).any() and any(not r.any() for r in flat)
    tabs = _tables(length, specs)
    want_pts, want_max, want_tok = joint_tokens(hm, 4, tabs)
    d_hm = torch.from_numpy(hm).cuda()
    w_pts, pts = _guarded((S, J, 2), torch.float32)
    w_max, mx = _guarded((S, J), torch.float32)
    dev, wholes = [], []
    for t in tabs:
        w_tok, tok = _guarded((t["n_grp"], t["K"]), torch.int32)
        wholes.append(w_tok)
        dev.append((tok, torch.tensor(t["group"], dtype=torch.int32, device="cuda"), torch.tensor(t["slot"], dtype=torch.int32, device="cuda")))
    a = _args(d_hm, pts, mx, tabs, dev)
    cabi.check(cabi.lib().i2r_joint_tokens(ctypes.byref(a), _stream()), "i2r_joint_tokens")
    torch.cuda.synchronize()
    assert np.array_equal(pts.cpu().numpy(), want_pts), "points"
    assert np.array_equal(mx.cpu().numpy(), want_max), "maxvals"
    for (tok, _, _), want in zip(dev, want_tok):
        got = tok.cpu().numpy()
        assert np.array_equal(got, want), "tokens: %d entries differ" % int((got != want).sum())
        assert not (got == I_POISON).any() and ((got == -1) == (want == -1)).all(), "an unwritten entry is not -1"
    assert any((w == -1).any() for w in want_tok) or case not in ("6x17x16x12-images-1-3-2", "2x17x64x48-two-tables")
    assert all(_canaries_intact(w) for w in [w_pts, w_max] + wholes), "a store outside a buffer"
    # the optional outputs left out: the tables alone, the same
    for tok, _, _ in dev:
        tok.fill_(I_POISON)
    a = _args(d_hm, None, None, tabs, dev)
    cabi.check(cabi.lib().i2r_joint_tokens(ctypes.byref(a), _stream()), "i2r_joint_tokens")
    torch.cuda.synchronize()
    assert all(np.array_equal(tok.cpu().numpy(), want) for (tok, _, _), want in zip(dev, want_tok))
    assert all(_canaries_intact(w) for w in wholes)


def test_raw_skips_crops_whose_device_table_is_wrong():
    """a group outside the table, a negative slot, a slot that does not fit the row: no store for that crop, the others as usual"""
    S, J, hh, hw = 4, 3, 4, 4
    hm = edge_maps(S, J, hh, hw, 5)
    spec = dict(n_grp=2, K=6, fh=4, fw=4, down=4, group=[0, 2, 1, 1], slot=[1, 0, -1, 2])
    good = dict(spec, group=[0, 0, 0, 0], slot=[1, 1, 1, 1])
    want = np.full((2, 6), -1, dtype=np.int32)
    want[0, 3:6] = joint_tokens(hm[:1], 4, [dict(good, group=[0], slot=[1])])[2][0][0, 3:6]
    w_tok, tok = _guarded((2, 6), torch.int32)
    dev = [(tok, torch.tensor(spec["group"], dtype=torch.int32, device="cuda"), torch.tensor(spec["slot"], dtype=torch.int32, device="cuda"))]
    a = _args(torch.from_numpy(hm).cuda(), None, None, [spec], dev)
    cabi.check(cabi.lib().i2r_joint_tokens(ctypes.byref(a), _stream()), "i2r_joint_tokens")
    torch.cuda.synchronize()
    assert np.array_equal(tok.cpu().numpy(), want) and _canaries_intact(w_tok)


def test_raw_rejects_bad_arguments():
    L = cabi.lib()
    S, J, hh, hw = 2, 3, 4, 4
    hm = torch.zeros(S, J, hh, hw, device="cuda")
    w_pts, pts = _guarded((S, J, 2), torch.float32)
    w_max, mx = _guarded((S, J), torch.float32)
    w_tok, tok = _guarded((2, 3), torch.int32)
    places = torch.zeros(2, S, dtype=torch.int32, device="cuda")
    tabs = [dict(n_grp=2, K=3, fh=2, fw=2, down=8)]
    dev = [(tok, places[0], places[1])]
    assert L.i2r_joint_tokens(None, None) == -1 and b"null pointer" in L.i2r_last_error()
    for kw, msg in ((dict(heatmaps=None), b"null pointer"), (dict(t0_tokens=None), b"null pointer"), (dict(t0_crop_group=None), b"null pointer"),
                    (dict(t0_crop_slot=None), b"null pointer"), (dict(n_crops=0), b"n_crops=0"), (dict(joints=0), b"joints=0"),
                    (dict(hh=0), b"heatmap 0x4"), (dict(hw=-1), b"heatmap 4x-1"), (dict(in_stride=0), b"in_stride=0"),
                    (dict(t0_fh=0), b"token map 0x2"), (dict(t0_fw=0), b"token map 2x0"), (dict(t0_down=0), b"down=0"), (dict(t0_n_grp=0), b"n_grp=0"),
                    (dict(t0_K=2), b"K=2 < joints=3"), (dict(n_tables=3), b"n_tables=3"), (dict(n_tables=-1), b"n_tables=-1"),
                    (dict(n_crops=1 << 16, joints=1 << 15, t0_K=1 << 15), b"exceed the grid limit"),
                    (dict(hh=1 << 16, hw=1 << 15), b"exceeds the index range")):
        a = _args(hm, pts, mx, tabs, dev, **kw)
        assert L.i2r_joint_tokens(ctypes.byref(a), _stream()) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    a = _args(hm, None, None, [], [])  # nothing to write at all
    assert L.i2r_joint_tokens(ctypes.byref(a), _stream()) == -1 and b"no output" in L.i2r_last_error()
    torch.cuda.synchronize()
    assert (pts == F_POISON).all() and (mx == F_POISON).all() and (tok == I_POISON).all(), "a rejected call launched or set something"
    assert all(_canaries_intact(w) for w in (w_pts, w_max, w_tok))


# ---------------------------------------------------------------------------------------------------------------------------------
# through attention_at_joints
# ---------------------------------------------------------------------------------------------------------------------------------
def _net(cfg, sd, precision="fp32"):
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    if precision != "fp32":
        net.set_precision(precision)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _case(tag):
    cfg, sd, x, m, length, _ = setup(tag)
    return cfg, sd, x, m, length


def _multi(y):
    return y["multi"] if isinstance(y, dict) else y


def _argmax_joints(multi):
    """4 x the torch arg-max (first index) of every map, (0, 0) where the maximum is not positive; and the maxima"""
    S, J, hh, hw = multi.shape
    flat = multi.reshape(S, J, -1)
    top, idx = flat.amax(-1), flat.argmax(-1)
    idx = torch.where(top > 0, idx, torch.zeros_like(idx))
    return 4.0 * torch.stack([idx % hw, idx // hw], -1).float(), top


def _same_output(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    return torch.equal(a, b)


def _compare_maps(got, ref, tol=None):
    assert set(got) == set(ref) and got
    worst = 0.0
    for key in got:
        a, b = (got[key], ref[key]) if isinstance(got[key], list) else ([got[key]], [ref[key]])
        assert len(a) == len(b)
        for u, v in zip(a, b):
            assert u.shape == v.shape, (key, u.shape, v.shape)
            if tol is None:
                assert torch.equal(u, v), "%s: %d entries differ, max-abs %.2e" % (key, int((u != v).sum()), (u - v).abs().max().item())
            else:
                worst = max(worst, (u - v).abs().max().item())
    return worst


@pytest.mark.parametrize("tag,precision", [("w48_l31", "fp32"), ("tph_l21", "fp32"), ("hrt_pre_nh2_l21", "fp32"), ("tph_l21", "bf16")])
def test_joints_call_equals_the_two_call_flow_bitwise(tag, precision):
    """the same launches on the same q|k with the same tables, no atomics: output, joints and maps are torch.equal to forward + host
    arg-max + attention_at -- inter-human stack only (w48), intra + inter (tph), the general layer's own q|k (hrt_pre_nh2)"""
    cfg, sd, x, m, length = _case(tag)
    net = _net(cfg, sd, precision)
    xd, md = x.cuda(), m.cuda()
    J = cfg.MODEL.NUM_JOINTS
    ups = (True, 1) if (tag, precision) == ("tph_l21", "fp32") else (True,)
    for mode in ("dependency", "affect"):
        for up in ups if mode == "dependency" else (True,):
            out, joints, maxvals, maps = net.attention_at_joints(xd, md, length, mode=mode, upsample=up)
            assert joints.is_cuda and maxvals.is_cuda and joints.shape == (sum(length), J, 2) and maxvals.shape == (sum(length), J)
            want, top = _argmax_joints(_multi(out))
            assert torch.equal(joints, want) and torch.equal(maxvals, top)
            out2, ref = net.attention_at(xd, md, length, joints.cpu(), mode=mode, upsample=up)
            torch.cuda.synchronize()
            assert _same_output(out, out2) and _same_output(out, net(xd, md, length))
            _compare_maps(maps, ref)
            for (st, _), v in maps.items():
                fh, fw = net.engine().capture_map_sizes(x.shape[2], x.shape[3])[st]
                r = x.shape[2] // fh if up is True else 1
                if st.startswith("singleformer."):
                    assert tuple(v.shape) == (sum(length), J, 1, fh * r, fw * r)
                else:
                    assert [tuple(t.shape) for t in v] == [(n * J, n, fh * r, fw * r) for n in length]
    assert set(maps) == {(st, i) for st, n in net.engine().capture_stacks().items() for i in range(n)}


@pytest.mark.parametrize("tag", ["w48_l31", "tph_l21", "hrt_pre_nh2_l21"])
def test_joints_call_under_the_flip_test(tag):
    """fp32: output = forward_flip's, joints = the arg-max of the MERGED maps, maps = the plain pass's at those joints -- within 2e-5 of
    attention_at on the plain program (the bar between two capture programs, tests/test_attn_query_gpu.py)"""
    cfg, sd, x, m, length = _case(tag)
    net = _net(cfg, sd)
    xd, md = x.cuda(), m.cuda()
    pairs = caller.FLIP_PAIRS["crowdpose" if cfg.MODEL.NUM_JOINTS == 14 else "coco"]
    out, joints, maxvals, maps = net.attention_at_joints(xd, md, length, upsample=1, flip_pairs=pairs)
    assert torch.is_tensor(out) and torch.equal(out, net.forward_flip(xd, md, length, pairs))
    want, top = _argmax_joints(out)
    assert torch.equal(joints, want) and torch.equal(maxvals, top)
    _, ref = net.attention_at(xd, md, length, joints.cpu(), upsample=1)
    torch.cuda.synchronize()
    worst = _compare_maps(maps, ref, tol=2e-5)
    print("%s flip: max-abs vs the plain program %.2e" % (tag, worst))
    assert worst <= 2e-5
    _, layer = net.attention_at_joints(xd, md, length, layers={sorted(maps)[-1]}, upsample=1, flip_pairs=pairs)[3].popitem()
    assert _compare_maps({0: layer}, {0: maps[sorted(maps)[-1]]}) == 0.0  # (one layer alone: the same launch on the same q|k)


def test_program_cache_and_hooks():
    """length [4, 4, 3] (capacity 12: one padding slot), then other inputs grouped [1, 2, 3, 5]: one joint program, nothing built for the
    second call, the default and full-capture programs stay, no hook is called"""
    cfg = config.load_config("w48_pure_en6")
    sd = synth.make_state_dict([(k, s, d) for k, (s, d) in keys_manifest("w48_pure_en6").items()])
    net = _net(cfg, sd)
    eng = net.engine()
    x, m, length = synth.make_inputs([4, 4, 3], 256, 192)
    xd, md = x.cuda(), m.cuda()
    y0 = net(xd, md, length).clone()
    rec = []
    hook = net.global_encoder.layers[0].self_attn.register_forward_hook(lambda mod, inp, out: rec.append(out[1]))
    net(xd, md, length)
    keys0 = set(eng.programs)
    assert len(keys0) == 2 and sum(1 for k in keys0 if "capture" in k) == 1 and len(rec) == 1
    out, joints, _, maps = net.attention_at_joints(xd, md, length, mode="affect", upsample=2)
    assert torch.equal(out, y0) and torch.equal(joints, _argmax_joints(out)[0])
    builds = eng.n_builds
    key = [k for k in eng.programs if "joints" in k]
    assert len(key) == 1 and key[0][-1] == "joints" and "query" in key[0] and cfg.MODEL.NUM_JOINTS in key[0]
    prog = eng.programs[key[0]][0]
    first = maps[("global_encoder", 5)][0].clone()
    x2, m2, length2 = synth.make_inputs([1, 2, 3, 5], 256, 192)
    out2, joints2, _, maps2 = net.attention_at_joints(x2.cuda(), m2.cuda(), length2, mode="affect", upsample=2)
    torch.cuda.synchronize()
    assert eng.n_builds == builds and eng.programs[key[0]][0] is prog, "other inputs or a regroup at the same capacity rebuilt the program"
    assert sum(1 for k in eng.programs if "joints" in k) == 1 and keys0 < set(eng.programs) and len(eng.programs) == 3
    J = cfg.MODEL.NUM_JOINTS
    assert out2.shape[0] == 11 and torch.equal(joints2, _argmax_joints(out2)[0])
    assert [tuple(v.shape) for v in maps2[("global_encoder", 0)]] == [(n * J, n, 32, 24) for n in length2]
    assert first.shape == (4 * J, 4, 32, 24) and maps2[("global_encoder", 5)][0].shape == (J, 1, 32, 24)
    assert len(rec) == 1, "attention_at_joints served forward hooks"
    hook.remove()
    assert torch.equal(net(xd, md, length), y0) and eng.n_builds == builds


def test_refusals():
    cfg, sd, x, m, length = _case("w48_l31")
    net = _net(cfg, sd)
    eng = net.engine()
    xd, md = x.cuda(), m.cuda()
    cap = {("global_encoder", 0)}
    tokens = {"global_encoder": torch.zeros(len(length), 1, dtype=torch.int32)}
    with pytest.raises(ValueError, match="not with"):
        eng.forward(xd, md, length, capture=cap, joints=JointQueries(), queries=AttnQueries(tokens))
    with pytest.raises(ValueError, match="not with"):
        eng.forward(xd, md, length, capture=cap, joints=JointQueries(), persons=PersonMaps())
    with pytest.raises(ValueError, match="needs capture"):
        eng.forward(xd, md, length, joints=JointQueries())
    with pytest.raises(ValueError, match="encoder stacks are"):
        net.attention_at_joints(xd, md, length, layers={("global_encoder", 6)})
    with pytest.raises(ValueError, match="mode"):
        net.attention_at_joints(xd, md, length, mode="both")
    assert not eng.programs, "a refused call built a program"
    # the existing refusals with the flip test stay
    jm = caller.joint_map(caller.FLIP_PAIRS["crowdpose"], cfg.MODEL.NUM_JOINTS).cuda()
    with pytest.raises(AssertionError):
        eng.forward(xd, md, length, flip_joint_map=jm, capture=cap, queries=AttnQueries(tokens))
    with pytest.raises(ValueError, match="not with"):
        eng.forward(xd, md, length, flip_joint_map=jm, capture=cap, persons=PersonMaps())
    # the window-type block
    cfg, sd, x, m, length = _case("bare_win_l213")
    with pytest.raises(ValueError, match="ATTENTION_TYPE window"):
        _net(cfg, sd).attention_at_joints(x.cuda(), m.cuda(), length)
    # a model without encoder stacks: the stand-alone HRFormer stage
    cfg, sd, x, m, length = _case("hrt_pre_nh2_l21")
    body = {k[len("singleformer."):]: v for k, v in sd.items() if k.startswith("singleformer.")}
    single = models.hrformer.get_pose_net(cfg, False, cfg.MODEL.SINGLE_MODEL, cfg.MODEL.END2END)
    single.load_state_dict(body, strict=True)
    with pytest.raises(ValueError):
        single.cuda().attention_at_joints(x.cuda(), m.cuda(), length)
