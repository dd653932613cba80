"""-m gpu: the fp32 HRFormer-B path against float64 at its edges, on poisoned buffers (cases: tests/_hrformer_cases.py).

Every program here is a tracked_program run through run_poisoned (tests/_gpu_util.py): all activation buffers but the loaded inputs
hold NaN before the first run; every output must come out finite over its whole extent with pad channels (and pad head dims) exactly
zero, and a second run over the leftovers must reproduce the first bit for bit.  Each test prints its GPU error next to the error of
the plain fp32 torch restatement of the same case, both against float64 (lines starting with HRF-ERR).

Measured on MI355X when the file was written, max-abs against float64 over the fp32 cases of a group (fp32 torch in brackets); every
case passed, and the bounds stay the project's, not these figures:
  LayerNorm 1.7e-7 .. 1.4e-6 (1.5e-7 .. 1.6e-6), bound 2e-5          window attention 3.1e-7 .. 2.8e-6 (3.2e-7 .. 2.5e-6), bound 2e-4
  dwconv 1.5e-8 .. 4.2e-7 (1.5e-8 .. 6.2e-7), bound 5e-5             upsample 6.0e-8 .. 3.8e-7 (6.0e-8 .. 9.0e-7), bounds 1e-5 / 2e-5
  blocks 1.1e-6 .. 3.0e-6 (7.0e-7 .. 2.4e-6), bound 2e-4             modules 1.5e-6 .. 2.7e-6 (1.4e-6 .. 3.0e-6), bound 1e-3
  16-bit storage: LayerNorm 7.8e-3 bf16 / 9.7e-4 f16, dwconv 3.9e-3 bf16 / 4.9e-4 f16, each within one rounding of the float64 value."""
import ctypes as C

import pytest
import torch

import _hrformer_cases as hc
from _gpu_util import act_nchw, run_poisoned, to_act, tracked_program
from i2r_amd import cabi, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ID = dict(ids=lambda c: c.id)


def _err(a, b):
    return (a.double() - b.double()).abs().max().item()


# ---------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.LN_CASES, **_ID)
def test_layernorm_matches_float64(case):
    dev = torch.device(DEV)
    x, w, b = hc.ln_tensors(case)
    ref = hc.ln_ref(x.double(), w.double(), b.double())
    P = tracked_program(dev)
    xa = to_act(P, x)
    out = P.layernorm(xa, engine.Packer({"n.weight": w, "n.bias": b}, dev).ln("n", case.c), out_dt=case.out_dt)
    assert out.dt == case.out_dt and out.cs == hc.ln_launch(case)["cs"]
    got = act_nchw(out, run_poisoned(P, [xa], [out])[0])
    e32 = _err(hc.ln_fp32(x, w, b), ref)
    hc.report("ln", case.id, _err(got, ref), e32, hc.TOL_LN)
    if case.out_dt:
        assert ((got.double() - ref).abs() <= hc.storage_bound(ref, case.out_dt)).all()
    else:
        assert _err(got, ref) < hc.TOL_LN


@pytest.mark.parametrize("case", hc.WA_CASES, **_ID)
def test_window_attention_matches_float64_loop_form(case):
    dev = torch.device(DEV)
    qkv, bias = hc.wa_tensors(case)
    ref = hc.window_attention_loop(qkv.double(), bias.double(), case.heads, case.hd)
    L = hc.wa_launch(case)
    P = tracked_program(dev)
    qa = P.alloc(case.n, case.h, case.w, 3 * L["hs"])
    assert qa.cs == 3 * L["hs"]
    qa.view().copy_(qkv.to(dev))
    out = P.winattn(qa, bias.to(dev), L["c"], case.heads)
    assert (out.c, out.cs) == (L["hs"], L["hs"])
    got = run_poisoned(P, [qa], [out], hd=case.hd)[0].cpu()
    e32 = _err(hc.window_attention_loop(qkv, bias, case.heads, case.hd), ref)
    hc.report("winattn", case.id, _err(got, ref), e32, hc.TOL_ATTN)
    assert _err(got, ref) < hc.TOL_ATTN


@pytest.mark.parametrize("case", hc.DW_CASES, **_ID)
def test_dwconv_matches_float64(case):
    dev = torch.device(DEV)
    x, sd = hc.dw_tensors(case)
    ref = hc.dw_ref(x.double(), sd, case.stride, case.act)
    P = tracked_program(dev)
    xa = to_act(P, x, case.dt)
    out = P.dwconv(xa, engine.Packer(sd, dev).dw("d", "b" if case.bn else None), case.stride, case.act)
    L = hc.dw_launch(case)
    assert (out.h, out.w, out.cs, out.dt) == (L["out_h"], L["out_w"], L["cs"], case.dt)
    got = act_nchw(out, run_poisoned(P, [xa], [out])[0])
    e32 = _err(hc.dw_ref(x, sd, case.stride, case.act), ref)
    hc.report("dwconv", case.id, _err(got, ref), e32, hc.TOL_DW)
    if case.dt:
        assert ((got.double() - ref).abs() <= hc.storage_bound(ref, case.dt)).all()
    else:
        assert _err(got, ref) < hc.TOL_DW


@pytest.mark.parametrize("case", hc.UP_CASES, **_ID)
def test_upsample_add_matches_float64(case):
    dev = torch.device(DEV)
    res, lows = hc.up_tensors(case)
    ref = hc.up_ref(res.double(), [t.double() for t in lows], case.scales, case.act)
    P = tracked_program(dev)
    ra, la = to_act(P, res), [to_act(P, t) for t in lows]
    one = ra if case.alias else P.alloc(case.n, case.H, case.W, case.c)
    P.upsample_add(la if len(la) > 1 else la[0], ra, one, act=case.act)
    outs, inputs = [one], [ra] + la
    if len(la) > 1:   # one pass per term, handing the fp32 sum through memory: bit-identical to the single pass
        r2 = to_act(P, res)
        seq = r2 if case.alias else P.alloc(case.n, case.H, case.W, case.c)
        for i, t in enumerate(la):
            P.upsample_add(t, r2 if i == 0 else seq, seq, act=case.act if i + 1 == len(la) else 0)
        outs.append(seq)
        inputs.append(r2)
    views = run_poisoned(P, inputs, outs)
    got = act_nchw(one, views[0])
    e32 = _err(hc.up_fp32(res, lows, case.scales, case.act), ref)
    hc.report("upsample", case.id, _err(got, ref), e32, hc.up_tol(case))
    assert _err(got, ref) < hc.up_tol(case)
    if len(la) > 1:
        assert torch.equal(views[0], views[1])


# ---------------------------------------------------------------------------------------------------------
# blocks and modules
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hc.BLOCK_CASES, **_ID)
def test_block_matches_float64_oracle(case):
    """HRFormerB._module (one branch, one block) + _emit_block against oracle.transformer_block in float64"""
    dev = torch.device(DEV)
    sd, st, x, ref, e32 = hc.block_reference(case)
    mod = engine.HRFormerB._module(engine.Packer(sd, dev), "m", st, True)
    P = tracked_program(dev)
    xa = to_act(P, x)
    out = engine.HRFormerB._emit_block(P, mod["blocks"][0][0], xa)
    kinds = [k for k, _, _ in P.ops]
    assert kinds.count(cabi.OP_LAYERNORM) == 2 and kinds.count(cabi.OP_WINATTN) == 1 and kinds.count(cabi.OP_DWCONV) == 1
    got = act_nchw(out, run_poisoned(P, [xa], [out])[0])
    hc.report("block", case.id, _err(got, ref), e32, hc.TOL_BLOCK)
    assert _err(got, ref) < hc.TOL_BLOCK


def _run_module(case, mods, xs, mode):
    """mode 0: lanes=False; 1: lanes=True, every lane on the caller's stream; 2: lanes=True between fork and join on the lane streams"""
    dev = torch.device(DEV)
    P = tracked_program(dev)
    xa = [to_act(P, x) for x in xs]
    mask = ((1 << case.nb) - 1) & ~1   # as HRFormerB.emit forks a stage: one region for all its modules
    if mode:
        P.fork(mask)
    ys = xa
    for mod in mods:
        ys = engine.HRFormerB._emit_module(P, mod, ys, mode != 0)
    if mode:
        P.join(mask)
    side = engine.lane_streams(dev, 3) if mode == 2 else None
    views = run_poisoned(P, xa, ys, side_streams=side)
    return [act_nchw(y, v) for y, v in zip(ys, views)]


@pytest.mark.parametrize("case", hc.MODULE_CASES, **_ID)
def test_module_matches_float64_oracle_on_every_schedule(case):
    """HRFormerB._module + _emit_module against oracle.hr_transformer_module in float64: without lanes, with lanes on one stream, and with
    lanes on the lane streams in whatever synchronisation form run() picks -- the three agree bit for bit"""
    dev = torch.device(DEV)
    sd, st, xs, refs, e32 = hc.module_reference(case)
    pk = engine.Packer(sd, dev)
    mods = [engine.HRFormerB._module(pk, q, st, case.multiscale) for q in hc.module_keys(case.mods)]
    assert mods[-1]["n_out"] == len(refs)
    got = [_run_module(case, mods, xs, mode) for mode in (0, 1, 2)]
    for mode, name in enumerate(("plain", "lanes-1stream", "lanes-streams")):
        err = max(_err(g, r) for g, r in zip(got[mode], refs))
        hc.report("module", "%s/%s" % (case.id, name), err, e32, hc.TOL_MODULE)
    for mode in (0, 1, 2):
        assert len(got[mode]) == len(refs)
        for g, r in zip(got[mode], refs):
            assert g.shape == r.shape and _err(g, r) < hc.TOL_MODULE
    for mode in (1, 2):
        assert all(torch.equal(a, b) for a, b in zip(got[0], got[mode])), "schedule %d differs from the plain one" % mode


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_tower_reproduces_itself_on_a_poisoned_arena(precision, monkeypatch):
    """the stand-alone HRFormer-B first stage (stem, layer1, transitions, all modules on their lanes, head): after one forward every
    activation buffer of its program is filled with NaN; the next forward -- the input is bound per call -- gives the same finite
    features and heat maps bit for bit, so no producer of the tower relies on what a buffer held before"""
    import numpy as np
    from _golden import setup
    from _gpu_util import NAN_WORD
    from i2r_amd import models
    alloc = engine.Program.alloc

    def alloc_tracked(self, *args, **kw):
        a = alloc(self, *args, **kw)
        acts = self.__dict__.setdefault("acts", [])
        if all(a.t is not t for t in acts):
            acts.append(a.t)
        return a
    monkeypatch.setattr(engine.Program, "alloc", alloc_tracked)
    cfg, sd, x, m, length, g = setup("hrt_l21")
    body = {k[len("singleformer."):]: v for k, v in sd.items() if k.startswith("singleformer.")}
    net = models.hrformer.get_pose_net(cfg, False, cfg.MODEL.SINGLE_MODEL, cfg.MODEL.END2END)
    net.load_state_dict(body, strict=True)
    net = net.cuda().set_precision(precision)
    xd = x.cuda()
    feat, hm = [t.clone() for t in net(xd)]
    torch.cuda.synchronize()
    progs = [v[0] for v in net.engine().programs.values()]
    assert len(progs) == 1 and len(progs[0].acts) > 20 and progs[0].uses_lanes
    for t in progs[0].acts:
        t.view(torch.int32).fill_(NAN_WORD)
    feat2, hm2 = net(xd)
    torch.cuda.synchronize()
    assert not progs[0].sync_timed_out()
    assert torch.isfinite(feat2).all() and torch.isfinite(hm2).all()
    assert torch.equal(feat, feat2) and torch.equal(hm, hm2)
    if precision == "fp32":
        assert np.abs(hm2.cpu().numpy() - g["out_single"]).max() < 1e-3


def test_poisoning_catches_a_buffer_nobody_writes():
    """the helper itself: an output that no launch writes, and one whose pad channels were loaded non-zero, do not pass"""
    dev = torch.device(DEV)
    x, w, b = hc.ln_tensors(hc.LN_CASES[1])
    ln = engine.Packer({"n.weight": w, "n.bias": b}, dev).ln("n", 78)
    P = tracked_program(dev)
    xa = to_act(P, x)
    out = P.layernorm(xa, ln)
    orphan = P.alloc(xa.n, xa.h, xa.w, xa.c)
    with pytest.raises(AssertionError, match="non-finite"):
        run_poisoned(P, [xa], [out, orphan])
    P = tracked_program(dev)
    xa = to_act(P, x)
    xa.view()[..., 78:] = 1.0   # a producer that left something in its pad channels: LayerNorm's mean takes it in, its w = b = 0 hide it ...
    low = to_act(P, x)
    y = P.alloc(xa.n, xa.h, xa.w, xa.c)
    P.upsample_add(low, xa, y, act=0)   # ... this pass (scale 1) carries it through
    with pytest.raises(AssertionError, match="pad channels"):
        run_poisoned(P, [xa, low], [y])


# ---------------------------------------------------------------------------------------------------------
# argument rejection through the raw C ABI: -1, nothing launched, i2r_last_error() names the function
# ---------------------------------------------------------------------------------------------------------
def test_raw_cabi_rejects_what_the_kernels_cannot_do():
    L = cabi.lib()
    dev = torch.device(DEV)
    a, b, c, d = (torch.zeros(4096, device=dev) for _ in range(4))
    pa, pb, pc, pd = (t.data_ptr() for t in (a, b, c, d))

    def rejected(rc, name):
        assert rc == -1, rc
        msg = L.i2r_last_error()
        assert msg and name in msg, msg

    for cs in (644, 648):   # past the ten register chunks of a lane (cs <= 640)
        rejected(L.i2r_layernorm(pa, pb, pc, pd, 1, cs, cs, 1e-6, 0, None), b"i2r_layernorm")
    rejected(L.i2r_window_attn(pa, pb, pc, 1, 1, 1, 72, 80, 2, None), b"i2r_window_attn")     # head_dim 36
    rejected(L.i2r_window_attn(pa, pb, pc, 1, 1, 1, 82, 80, 2, None), b"i2r_window_attn")     # head_dim 41
    rejected(L.i2r_window_attn(pa, pb, pc, 1, 1, 1, 78, 78, 2, None), b"i2r_window_attn")     # hs != heads*40
    rejected(L.i2r_window_attn(pa, pb, pc, 1, 1, 1, 78, 96, 2, None), b"i2r_window_attn")
    rejected(L.i2r_dwconv3x3(pa, pb, pc, pd, 1, 4, 4, 78, 80, 2, 0, 1, None), b"i2r_dwconv3x3")  # 16-bit storage, stride 2
    rejected(L.i2r_dwconv3x3(pa, pb, pc, pa, 1, 4, 4, 78, 80, 1, 0, 0, None), b"i2r_dwconv3x3")  # in == out
    up = cabi.UpArgs(pa, pb, pc, 1, 2, 2, 2, 78, 80, 0, pd, None, 3, 1)                           # 4x4 output, second scale 3
    rejected(L.i2r_upsample_bilinear_add_multi(C.byref(up), None), b"i2r_upsample_bilinear_add")
    up = cabi.UpArgs(pa, pb, pc, 1, 2, 2, 2, 78, 80, 0, None, pd, 1, 2)                           # low3 without low2
    rejected(L.i2r_upsample_bilinear_add_multi(C.byref(up), None), b"i2r_upsample_bilinear_add")
    torch.cuda.synchronize()
    assert all(t.abs().sum().item() == 0.0 for t in (a, b, c, d))   # nothing ran
