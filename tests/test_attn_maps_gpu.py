"""-m gpu: attention maps on the MI355X -- the raw i2r_attn_weights C-ABI against float64 torch, the forward-hook path of every model
kind against the CPU restatement (tests/_attn_ref.py) and the reference's own hook rows (tests/golden/attn_*.npz), regrouping on one
capture program, non-interference with the default forward, and the 16-bit modes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _attn_ref import restate
from _golden import GOLDEN, keys_manifest, setup
from i2r_amd import arch, cabi, config, models, synth

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
# raw C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
LENS = [17, 768, 1, 3072, 5, 192, 1152, 16]
CANARY = 12345.0


@pytest.mark.parametrize("heads,hp", [(1, 96), (1, 80), (2, 48), (4, 32), (8, 16)])
def test_raw_attn_weights_match_float64(heads, hp):
    g = torch.Generator(device="cuda").manual_seed(heads * 1000 + hp)
    hd = hp - 3 if hp > 16 else hp  # (pad dims of the head stay exactly 0)
    hs = heads * hp
    k_off = hs + 16
    qk_cs = k_off + hs + 8
    lens = LENS + [40]  # the last group is in the offset table but not computed (n_grp excludes it)
    n_tok = sum(lens)
    qk = torch.zeros(n_tok, qk_cs, device="cuda")
    for h in range(heads):
        qk[:, h * hp:h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g) * 2.0 * hd ** -0.5
        qk[:, k_off + h * hp:k_off + h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    # blocks with gaps of canaries between them (offsets not all multiples of 4: both store forms)
    out_off, pos = [], 7
    for n in LENS:
        out_off.append(pos)
        pos += n * n + 5
    total = pos + 64
    out = torch.full((total,), CANARY, device="cuda")
    goff = torch.tensor(offs, dtype=torch.int32, device="cuda")
    ooff = torch.tensor(out_off, dtype=torch.int64, device="cuda")
    nkb = max(-(-n // 128) for n in LENS)
    ws = torch.empty(n_tok * 2 * heads * nkb, device="cuda")
    a = cabi.AttnWeightsArgs(qk.data_ptr(), out.data_ptr(), goff.data_ptr(), ooff.data_ptr(), ws.data_ptr(), len(LENS), heads, hp, k_off,
                             qk_cs, sum(-(-n // 16) * -(-n // 128) for n in LENS), 2 * heads * nkb)
    cabi.check(cabi.lib().i2r_attn_weights(ctypes.byref(a), _stream()), "i2r_attn_weights")
    torch.cuda.synchronize()
    written = torch.zeros(total, dtype=torch.bool, device="cuda")
    for gi, n in enumerate(LENS):
        o = offs[gi]
        q = qk[o:o + n].double()
        ref = torch.zeros(n, n, dtype=torch.float64, device="cuda")
        for h in range(heads):
            s = q[:, h * hp:(h + 1) * hp] @ q[:, k_off + h * hp:k_off + (h + 1) * hp].t()
            ref += torch.softmax(s, dim=-1)
        ref /= heads
        got = out[out_off[gi]:out_off[gi] + n * n].view(n, n).double()
        err = (got - ref).abs().max().item()
        assert err <= 1e-5, "L=%d heads=%d hp=%d: max-abs %.2e" % (n, heads, hp, err)
        assert (got.sum(-1) - 1).abs().max().item() <= 1e-5
        written[out_off[gi]:out_off[gi] + n * n] = True
    assert (out[~written] == CANARY).all(), "a store outside the computed blocks"


def test_raw_attn_weights_rejects_bad_arguments():
    a = cabi.AttnWeightsArgs()
    assert cabi.lib().i2r_attn_weights(ctypes.byref(a), None) == -1
    assert b"null pointer" in cabi.lib().i2r_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# through the forward hooks
# ---------------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """the reference's recipe: hooks on every <stack>.layers[i].self_attn (output[1]) and on the reduce modules (output)"""

    def __init__(self, net):
        self.maps, self.feats, self.handles = {}, {}, []
        for st, i, m in net._attn_sites:
            self.handles.append(m.register_forward_hook(lambda mod, inp, out, k=(st, i): self.maps.setdefault(k, []).append(out[1])))
        for st, m in net._reduce_sites:
            self.handles.append(m.register_forward_hook(lambda mod, inp, out, k=st: self.feats.setdefault(k, []).append(out)))

    def remove(self):
        for h in self.handles:
            h.remove()


def _net(cfg, sd, precision="fp32"):
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    if precision != "fp32":
        net.set_precision(precision)
    return net.cuda()


def _check_maps(rec, maps, lens_of, tol, tag, fx=None):
    assert set(rec.maps) == set(maps), (sorted(rec.maps), sorted(maps))
    worst = 0.0
    for key, w_ref in maps.items():
        assert len(rec.maps[key]) == 1
        w = rec.maps[key][0].float().cpu()
        assert w.shape == w_ref.shape, (key, w.shape, w_ref.shape)
        for b, n in enumerate(lens_of(key[0])):
            assert not w[b, :, n:].any() and not w[b, n:].any(), "%s %s entry %d: padded rows / columns not exactly 0" % (tag, key, b)
            err = (w[b, :n, :n] - w_ref[b, :n, :n]).abs().max().item()
            worst = max(worst, err)
            assert err < tol, "%s %s entry %d: max-abs %.2e vs restatement" % (tag, key, b, err)
            assert (w[b, :n, :n].double().sum(-1) - 1).abs().max().item() < 1e-5
            if fx is not None and "%s.%d.%d.rows" % (key[0], key[1], b) in fx:
                rows = fx["%s.%d.%d.rows" % (key[0], key[1], b)]
                e2 = np.abs(w[b, torch.from_numpy(rows)].numpy() - fx["%s.%d.%d.maps" % (key[0], key[1], b)]).max()
                assert e2 < tol, "%s %s entry %d: max-abs %.2e vs the reference's hook rows" % (tag, key, b, e2)
    return worst


HOOK_TAGS = ["w48_l31", "tph_l21", "hrt_l21", "tph2s_l12", "bare_l21", "w48_nh8_l21", "hrt_pre_nh2_l21", "ochtph_cv_nh2_l21"]


@pytest.mark.parametrize("tag", HOOK_TAGS)
def test_hooked_forward_maps_match_restatement_and_reference(tag):
    cfg, sd, x, m, length, _ = setup(tag)
    net = _net(cfg, sd)
    rec = Recorder(net)
    net(x.cuda(), m.cuda(), length)
    torch.cuda.synchronize()
    rec.remove()
    maps, feats, _ = restate(cfg, sd, x, m, length)
    fpath = os.path.join(GOLDEN, "attn_%s.npz" % tag)
    fx = dict(np.load(fpath)) if os.path.exists(fpath) else None
    tok = {st: w.shape[1] // (max(length) if st != "singleformer.global_encoder" else 1) for (st, _), w in maps.items()}
    lens_of = lambda st: [tok[st]] * sum(length) if st == "singleformer.global_encoder" else [n * tok[st] for n in length]  # noqa: E731
    worst = _check_maps(rec, maps, lens_of, TOL, tag, fx)
    for st, got in rec.feats.items():
        assert len(got) == 1
        err = (got[0].cpu() - feats[st]).abs().max().item()
        assert err < TOL, "%s: %s reduce features max-abs %.2e" % (tag, st, err)
    print("%s: maps max-abs vs restatement %.2e" % (tag, worst))


def test_standalone_transpose_h_hooks():
    cfg = config.load_config("tph_192_p6_b4")
    sd = synth.make_state_dict(arch.transpose_h_spec(cfg, ""))
    net = models.transpose_h.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    x, _, _ = synth.make_inputs([2, 1], 256, 192)
    rec = Recorder(net)
    feat, hm = net(x.cuda())
    torch.cuda.synchronize()
    rec.remove()
    maps, feats, y = restate(cfg, sd, x, None, None, standalone_single=True)
    assert (hm.cpu() - y[1]).abs().max().item() < TOL
    hw = feat.shape[2] * feat.shape[3]
    worst = _check_maps(rec, maps, lambda st: [hw] * 3, TOL, "transpose_h")
    assert (rec.feats["global_encoder"][0].cpu() - feats["global_encoder"]).abs().max().item() < TOL
    print("transpose_h: maps max-abs vs restatement %.2e" % worst)


def test_regroup_on_one_capture_program():
    """length [4, 4, 3] (capacity 12: one padding slot) then [1, 2, 3, 5] on the same program: both right, no rebuild"""
    cfg = config.load_config("w48_pure_en6")
    sd = synth.make_state_dict([(k, s, d) for k, (s, d) in keys_manifest("w48_pure_en6").items()])
    net = _net(cfg, sd)
    rec = Recorder(net)
    eng = net.engine()
    for i, length in enumerate(([4, 4, 3], [1, 2, 3, 5])):
        x, m, length = synth.make_inputs(length, 256, 192)
        rec.maps.clear()
        rec.feats.clear()
        net(x.cuda(), m.cuda(), length)
        torch.cuda.synchronize()
        if i == 0:
            builds = eng.n_builds
        else:
            assert eng.n_builds == builds, "a regroup on the same capacity rebuilt the program"
        maps, feats, _ = restate(cfg, sd, x, m, length)
        _check_maps(rec, maps, lambda st: [n * 192 for n in length], TOL, "w48 %s" % length)
        assert (rec.feats["global_encoder"][0].cpu() - feats["global_encoder"]).abs().max().item() < TOL
    rec.remove()


def test_default_forward_is_untouched_by_hooks():
    cfg = config.load_config("w48_pure_en6")
    sd = synth.make_state_dict([(k, s, d) for k, (s, d) in keys_manifest("w48_pure_en6").items()])
    net = _net(cfg, sd)
    x, m, length = synth.make_inputs([3, 4, 2, 5, 4, 3, 5], 256, 192)  # 26 crops: the default path splits into part-batches
    x, m = x.cuda(), m.cuda()
    y0 = net(x, m, length).clone()
    eng = net.engine()
    keys0 = set(eng.programs)
    rec = Recorder(net)
    yh = net(x, m, length).clone()
    yh2 = net(x, m, length).clone()
    assert torch.equal(yh, yh2)
    rec.remove()
    y1 = net(x, m, length).clone()
    torch.cuda.synchronize()
    assert torch.equal(y0, y1), "the default forward changed after hooked forwards"
    assert (yh - y0).abs().max().item() < 1e-5
    assert {k for k in eng.programs if "capture" not in k} == keys0, "default program keys changed"
    assert len(rec.maps) == 6 and all(len(v) == 2 for v in rec.maps.values())


# 16-bit modes: the maps are computed in fp32 on the token rows the 16-bit layers received (fp32 in HBM).  Against the fp32 restatement
# they differ by what the 16-bit tower changed in those rows: mean-abs <= 1e-3 over every layer; for the first layer of each stack, whose
# input the capture returns, the maps equal the restatement on that very input (fp32 bar), and every entry stays inside the softmax bound
# |p' - p| <= p (exp(2 D) - 1) of the row's measured logit error D (attention maps).  A flat max-abs bar does not hold: a row
# with two near-equal logits moves by tenths when bf16 maps shift them by ~0.1.
LP_MEAN = 1e-3


def _logits(sd, p, t, n_head):
    """[B, L, d] q / k input -> [B, heads, L, L] logits of nn.MultiheadAttention (q scaled by head_dim^-0.5)"""
    d = t.shape[-1]
    hd = d // n_head
    w, b = sd[p + ".self_attn.in_proj_weight"].double(), sd[p + ".self_attn.in_proj_bias"].double()
    q = (t.double() @ w[:d].t() + b[:d]) * hd ** -0.5
    k = t.double() @ w[d:2 * d].t() + b[d:2 * d]
    B, L, _ = t.shape
    q, k = q.view(B, L, n_head, hd).transpose(1, 2), k.view(B, L, n_head, hd).transpose(1, 2)
    return q @ k.transpose(-1, -2)


@pytest.mark.parametrize("tag,precision", [("tph_l21", "bf16"), ("hrt_l21", "bf16"), ("hrt288_l2", "fp16")])
def test_16bit_maps(tag, precision):
    from _attn_ref import _stack_maps, _tokens
    import i2r_cpu
    cfg, sd, x, m, length, _ = setup(tag)
    M = cfg["MODEL"]
    net = _net(cfg, sd, precision)
    eng = net.engine()
    stacks = eng.capture_stacks()
    _, got = eng.forward(x.cuda(), m.cuda(), length, capture={(st, i) for st, n in stacks.items() for i in range(n)})
    torch.cuda.synchronize()
    maps, feats, _ = restate(cfg, sd, x, m, length)
    for key, w_ref in maps.items():
        st = key[0]
        single = st == "singleformer.global_encoder"
        tok = w_ref.shape[1] // (1 if single else max(length))
        lens = [tok] * sum(length) if single else [n * tok for n in length]
        mean = []
        for b, n in enumerate(lens):
            w = got[key][b].double().cpu()
            assert w.shape == (n, n) and (w.sum(-1) - 1).abs().max().item() < 1e-5
            mean.append((w - w_ref[b, :n, :n].double()).abs().mean().item())
        mx = max((got[key][b].cpu() - w_ref[b, :n, :n]).abs().max().item() for b, n in enumerate(lens))
        print("%s %s %s: max-abs %.3e mean-abs %.3e vs the fp32 restatement" % (tag, precision, key, mx, float(np.mean(mean))))
        assert float(np.mean(mean)) <= LP_MEAN, (key, float(np.mean(mean)))
        if key[1] != 0:
            continue
        # first layer: the capture's own input (what the 16-bit layer received) vs the fp32 oracle's
        f16 = got[(st, "input")].cpu()
        pos = sd[st.replace("global_encoder", "pos_embedding")].reshape(1, tok, -1).expand(f16.shape[0], -1, -1) if single else None
        assert single or not M["USE_MULTI_POS"]
        own = _stack_maps(sd, st, 1, [_tokens(f16)], pos, M["N_HEAD"], False, None if single else length)[(st, 0)]
        in_err = (f16 - feats[st]).abs().max().item()
        worst_own, worst_ratio = 0.0, 0.0
        for b, n in enumerate(lens):
            w = got[key][b].cpu()
            worst_own = max(worst_own, (w - own[b, :n, :n]).abs().max().item())
            # softmax bound from the logit error D_i of each row: |p' - p| <= p (exp(2 D_i) - 1)
            if single:
                t16, t32 = _tokens(f16[b:b + 1]) + pos[:1], _tokens(feats[st][b:b + 1]) + pos[:1]
            else:
                o = sum(length[:b])
                t16 = _tokens(f16[o:o + length[b]]).reshape(1, n, -1)
                t32 = _tokens(feats[st][o:o + length[b]]).reshape(1, n, -1)
            D = (_logits(sd, "%s.layers.0" % st, t16, M["N_HEAD"]) - _logits(sd, "%s.layers.0" % st, t32, M["N_HEAD"])).abs().amax(dim=(0, 1, 3))
            bound = w_ref[b, :n, :n].double() * torch.expm1(2 * D)[:, None] + 1e-4
            ratio = ((w.double() - w_ref[b, :n, :n].double()).abs() / bound).max().item()
            worst_ratio = max(worst_ratio, ratio)
        print("   layer-0 input max-abs err %.3e; maps vs the restatement on the layer's own input %.2e; worst |dp| / softmax bound %.3f"
              % (in_err, worst_own, worst_ratio))
        assert worst_own < 1e-4 and worst_ratio <= 1.0


def _flat(res):
    """every tensor of what a capture call returned (output, maps; PersonRelations), cloned, in a fixed order"""
    if torch.is_tensor(res):
        return [res.clone()]
    if isinstance(res, dict):
        return [t for k in sorted(res, key=str) for t in _flat(res[k])]
    if isinstance(res, (list, tuple)):
        return [t for r in res for t in _flat(r)]
    return _flat(res.relation) + _flat(res.maps)


def test_one_engine_serves_all_three_forms():
    """full capture, attention_at, person_relations and full capture again on ONE engine: every call gives the bits of the same call on a
    fresh engine, the heat maps stay the default forward's, and the four calls build exactly three programs"""
    cfg, sd, x, m, length, _ = setup("w48_l31")
    x, m = x.cuda(), m.cuda()
    pts = torch.tensor([[10.0, 20.0], [100.0, 200.0], [191.0, 255.0]]).repeat(x.shape[0], 1, 1)

    def calls(net):
        cap = {(net.engine().inter_stack, 0)}
        return [lambda: net.engine().forward(x, m, length, capture=cap),
                lambda: net.attention_at(x, m, length, pts, mode="affect", layers=cap),
                lambda: net.person_relations(x, m, length, layers=cap, maps="dependency", upsample=2),
                lambda: net.engine().forward(x, m, length, capture=cap)]

    net = _net(cfg, sd)
    y0 = net(x, m, length).clone()
    eng = net.engine()
    builds = eng.n_builds
    got = [_flat(fn()) for fn in calls(net)]
    assert eng.n_builds == builds + 3, "four calls in three forms: %d programs built" % (eng.n_builds - builds)
    for i, res in enumerate(got):
        assert torch.equal(res[0], y0), "call %d: heat maps differ from the default forward's" % i
        fresh = _flat(calls(_net(cfg, sd))[i]())
        assert len(res) == len(fresh) > 1 and all(torch.equal(a, b) for a, b in zip(res, fresh)), "call %d differs from a fresh engine's" % i
    assert all(torch.equal(a, b) for a, b in zip(got[0], got[3]))
