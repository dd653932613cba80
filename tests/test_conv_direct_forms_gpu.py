"""-m gpu: the body and epilogue forms of the direct fp32 conv (csrc/i2r_conv.hip: conv_igemm_f32<MT, NT, CAP, PF, FORM, EPI>; FORM 1 = the
single-chunk body, 2 = the pipelined body, EPI 1 = bias + ReLU, 2 = bias + res1 + ReLU), through the raw C-ABI with the helpers of
tests/_conv_cases.py.  Every launch runs with the forms on and off (i2r_conv_direct_forms) into outputs prefilled with NaN; the two
results are compared BIT FOR BIT, the switched-on one also against the float64 reference at the bar of
tests/test_kernels_gpu.py::test_conv_every_instantiation_matches_float64 (2e-5 * max(1, max |ref|)), and i2r_conv_direct_form must report
the (form, epi) the case was built for.  The shapes are the smallest that reach every path (tests/test_conv_direct_forms.py checks the
same table on the CPU: names and forms)."""
import ctypes as C

import pytest
import torch

import _conv_direct_cases as dc
import _conv_cases as cc
from i2r_amd import cabi, engine, models, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _switch(on):
    cabi.check(cabi.lib().i2r_conv_direct_forms(int(on)), "i2r_conv_direct_forms")


def _prefill(c, t, out):
    """NaN everywhere; a case that accumulates in place keeps its residual in the pixels and channels it owns"""
    out.fill_(NAN)
    if c.inplace:
        body = out[cc.GUARD:cc.GUARD + c.n * c.out_h].view(c.n, c.out_h, c.out_w, c.out_cs)
        own = cc.owned_mask(c).to(out.device)
        body[:, own, :c.cout] = t["res1"].to(out.device)[:, own, :c.cout]


def _launch(members, ts, bm, on):
    """-> ((form, epi), [guarded output buffer on the CPU per member]) of ONE launch with the switch at `on`"""
    dev = torch.device(DEV)
    _switch(on)
    try:
        args = [cc.launch_args(m, t, dev) for m, t in zip(members, ts)]
        for m, t, a in zip(members, ts, args):
            _prefill(m, t, a[1])
        descs = [a[0] for a in args]
        got = dc.direct_form(descs)
        arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
        bmd = torch.tensor(bm, dtype=torch.int32, device=dev) if bm is not None else None
        cabi.check(cabi.lib().i2r_conv_grouped(arr, len(descs), bmd.data_ptr() if bm is not None else None, len(bm) if bm is not None else 0,
                                               torch.cuda.current_stream(dev).cuda_stream), "i2r_conv_grouped")
        torch.cuda.synchronize()
        return got, [a[1].cpu() for a in args]
    finally:
        _switch(1)


def _check(c, t, buf, ref):
    """the switched-on result against float64; what the launch does not own is still NaN"""
    exp, own = ref
    g = buf.double()
    assert torch.isnan(g[:cc.GUARD]).all() and torch.isnan(g[-cc.GUARD:]).all(), "%s: guard rows written" % c.id
    body = g[cc.GUARD:-cc.GUARD].view(c.n, c.out_h, c.out_w, c.out_cs)
    assert torch.isnan(body[:, ~own]).all(), "%s: pixels the descriptor does not own were written" % c.id
    got, want = body[:, own][..., :c.cout], exp[:, own]
    assert not torch.isnan(got).any(), "%s: out not written completely" % c.id
    err, bar = (got - want).abs().max().item(), 2e-5 * max(1.0, want.abs().max().item())
    print("%s: max |got - ref| %.3e (bar %.3e)" % (c.id, err, bar))
    assert err < bar, "%s: max |got - ref| %.3e exceeds %.3e (%s)" % (c.id, err, bar, c.describe())
    if c.out_cs >= c.cout_pad:
        assert (body[:, own][..., c.cout:c.cout_pad] == 0.0).all(), "%s: padding channels must be exactly zero" % c.id
        assert torch.isnan(body[:, own][..., c.cout_pad:]).all(), "%s: channels past cout_pad written" % c.id


def _both(members, bm, name, want):
    ts = [cc.make_tensors(m) for m in members]
    rc, got_name, err = cc.resolve([m.desc() for m in members])
    assert rc == 0 and got_name == name, (got_name, err)
    f0, off = _launch(members, ts, bm, 0)
    f1, on = _launch(members, ts, bm, 1)
    assert f0 == (0, 0) and f1 == want, (f0, f1, want)
    for m, t, b0, b1 in zip(members, ts, off, on):
        _check(m, t, b1, cc.reference(m, t))
        assert torch.equal(b1.view(torch.int32), b0.view(torch.int32)), "%s: differs from the general body, max |d| %.3e" % (
            m.id, (b1 - b0).nan_to_num().abs().max().item())


@pytest.mark.parametrize("key", list(dc.SINGLES))
def test_single_launches_match_float64_and_the_general_body_bitwise(key):
    c, name, want = dc.SINGLES[key]
    _both([c], None, name, want)


@pytest.mark.parametrize("table", [False, True], ids=["nomap", "lpt"])
@pytest.mark.parametrize("key", list(dc.GROUPS))
def test_grouped_launches_match_float64_and_the_general_body_bitwise(key, table):
    members, name, want = dc.GROUPS[key]
    bm = engine.lpt_block_order(dc.counts(members), [m.cin * len(m.taps) for m in members]) if table else None
    _both(members, bm, name, want)


def _model(forms_on):
    saved = engine.CONV_FORMS
    engine.CONV_FORMS = forms_on
    try:
        from i2r_amd import arch, config
        cfg = config.load_config("w48_pure_en6")
        sd = synth.make_state_dict(arch.param_spec(cfg))
        x, m, length = synth.make_inputs([2, 2], 256, 192, seed=7)
        net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
        y = net(x.cuda(), m.cuda(), length).cpu()
        forms = set()
        for P, *_ in net.engine().programs.values():
            for k, _, st in P.ops:
                if k == cabi.OP_CONV_GROUP and st.d[0].contents.algo == 0:
                    forms.add(dc.direct_form([st.d[i].contents for i in range(st.n)]))
                elif k == cabi.OP_CONV and st.algo == 0:
                    forms.add(dc.direct_form([st]))
        return y, forms
    finally:
        engine.CONV_FORMS = saved
        engine.push_conv_forms()


def test_model_heat_maps_are_bitwise_equal_with_and_without_forms():
    """vanilla config, 2 images x 2 persons: with the switch off every direct conv reports (0, 0), with it on the tower's launches take the
    single-chunk and the pipelined body and both epilogue forms; the heat maps are the same bits"""
    y0, f0 = _model(False)
    y1, f1 = _model(True)
    assert f0 == {(0, 0)}, f0
    assert {f for f, _ in f1} >= {1, 2} and {e for _, e in f1} >= {1, 2}, f1
    assert torch.isfinite(y0).all() and torch.equal(y0, y1), "max |d| %.3e" % (y0 - y1).abs().max().item()
