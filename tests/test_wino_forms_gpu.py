"""-m gpu: the compile-time epilogue forms of the Winograd kernels (csrc/i2r_conv_wino.hip, EPI 1 = bias + ReLU, 2 = bias + res1 + ReLU).
Every launch is checked two ways: against float64 torch on the CPU at the project's bar 2e-5 * max(1, max |ref|)
(tests/test_kernels_gpu.py::test_conv_winograd_matches_torch_and_direct), and bit for bit against the same launch with the forms switched
off (i2r_conv_wino_forms(0): the general epilogue).  Outputs are prefilled with NaN.  The shapes are the smallest that reach every path:
fragments straddling crops, two channel blocks, NT = 4, a ragged map (pixels through the out-of-range offset), the fused-input staging,
a grouped launch with and without a dispatch table, a group that must fall back to the general form."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from _gpu_util import from_act, run, to_act
from i2r_amd import cabi, engine, models, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(29, key, tuple(shape), scale))


class Member:
    """one conv of a launch with its float64 reference: input (plus up-sampled terms at 1 / scales: the fused-input form), folded BN,
    residual in front of the ReLU (res1) or behind it (res_post)"""

    def __init__(self, n, cin, cout, h, w, tag, scales=(), res1=False, res_post=False, relu=True):
        self.scales, self.tag, self.relu = scales, tag, relu
        self.sd = {"c.weight": _rand((cout, cin, 3, 3), "w" + tag, (6.0 / (cin * 9)) ** 0.5),
                   "b.weight": _rand((cout,), "g" + tag, 0.5) + 1.0, "b.bias": _rand((cout,), "b" + tag, 0.3),
                   "b.running_mean": _rand((cout,), "m" + tag, 0.3), "b.running_var": _rand((cout,), "v" + tag, 0.4) + 1.0}
        self.base = _rand((n, cin, h, w), "x" + tag)
        self.terms = [_rand((n, cin, h // s, w // s), "t%d%s" % (s, tag)) for s in scales]
        self.res1 = _rand((n, cout, h, w), "r1" + tag) if res1 else None
        self.res_post = _rand((n, cout, h, w), "rp" + tag) if res_post else None
        y = self.base.double()
        for t, s in zip(self.terms, scales):
            y = y + F.interpolate(t.double(), scale_factor=s, mode="nearest")
        y = F.relu(y) if scales else y
        sd = {k: v.double() for k, v in self.sd.items()}
        ref = F.batch_norm(F.conv2d(y, sd["c.weight"], None, padding=1), sd["b.running_mean"], sd["b.running_var"], sd["b.weight"], sd["b.bias"], False, 0.0, 1e-5)
        if res1:
            ref = ref + self.res1.double()
        if relu:
            ref = F.relu(ref)
        if res_post:
            ref = ref + self.res_post.double()
        self.ref = ref

    def emit(self, P, grp):
        pc = engine.Packer(self.sd, torch.device(DEV)).conv("c", "b")
        base, terms = to_act(P, self.base), [to_act(P, t) for t in self.terms]
        kw = dict(relu=self.relu, group=grp, res1=to_act(P, self.res1) if self.res1 is not None else None,
                  res_post=to_act(P, self.res_post) if self.res_post is not None else None)
        self.y = None
        if self.scales:
            self.y = P.alloc(base.n, base.h, base.w, base.c)
            self.y.t.fill_(NAN)
            kw["fuse_in"] = (terms, self.y)
        self.out = P.conv(base, pc, **kw)
        self.out.t.fill_(NAN)


def _form(st):
    arr = (C.POINTER(cabi.ConvDesc) * st.n)(*[st.d[i] for i in range(st.n)])
    f = C.c_int32(-1)
    cabi.check(cabi.lib().i2r_conv_wino_form(arr, st.n, C.byref(f)), "i2r_conv_wino_form")
    return f.value


def _launch(ms, forms_on, seq=1, table=False):
    """-> (form the launch resolved to, [(y or None, out as stored, out NCHW float64)] per member) of ONE grouped launch"""
    saved = engine.WINO_FORMS
    engine.WINO_FORMS = forms_on
    try:
        dev = torch.device(DEV)
        P = engine.Program(dev)
        grp = []
        for m in ms:
            m.emit(P, grp)
        for g in grp:
            assert g[0].algo == 1
            g[0].seq = seq
        P.flush_group(grp)
        (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
        if table:  # the members interleaved, each walking its workgroups backwards
            arr = (C.POINTER(cabi.ConvDesc) * st.n)(*[st.d[i] for i in range(st.n)])
            total, seqs = C.c_int32(-1), (C.c_int32 * st.n)()
            left = []
            for i in range(st.n):  # workgroups per member: the grid of the member alone, with a table
                one = (C.POINTER(cabi.ConvDesc) * 1)(st.d[i])
                cabi.check(cabi.lib().i2r_conv_grid(one, 1, 1, C.byref(total), seqs), "i2r_conv_grid")
                left.append(total.value)
            order = []
            while any(left):
                for i in range(st.n):
                    if left[i]:
                        left[i] -= 1
                        order.append((i << 24) | left[i])
            cabi.check(cabi.lib().i2r_conv_grid(arr, st.n, 1, C.byref(total), seqs), "i2r_conv_grid")
            assert total.value == len(order)
            bm = torch.tensor(order, dtype=torch.int32, device=dev)
            P.keep.append(bm)
            st.block_map, st.map_len = bm.data_ptr(), bm.numel()
        else:
            st.block_map, st.map_len = None, 0
        engine.push_wino_forms()
        form = _form(st)
        run(P)
        return form, [(m.y.view().clone() if m.y is not None else None, m.out.view().clone(), from_act(m.out).double()) for m in ms]
    finally:
        engine.WINO_FORMS = saved
        engine.push_wino_forms()


_OFF = {}  # (case, seq, table) -> members with their float64 references + the results of the general form: computed once


def _both(name, make, want_form, seq=1, table=False):
    key = (name, seq, table)
    if key not in _OFF:
        ms = _OFF[(name, 1, False)][0] if (name, 1, False) in _OFF else make()
        f0, off = _launch(ms, False, seq, table)
        assert f0 == 0
        _OFF[key] = (ms, off)
    ms, off = _OFF[key]
    f1, on = _launch(ms, True, seq, table)
    assert f1 == want_form, (name, f1, want_form)
    for m, (y0, o0, _), (y1, o1, o64) in zip(ms, off, on):
        what = "%s %s seq %d%s" % (name, m.tag, seq, " table" if table else "")
        err, bar = (o64 - m.ref).abs().max().item(), 2e-5 * max(1.0, m.ref.abs().max().item())
        print("%s: form %d, max |got - ref| %.3e (bar %.3e)" % (what, f1, err, bar))
        assert not torch.isnan(o1[..., :m.out.c]).any(), "%s: out not written completely" % what
        assert err < bar, "%s: max-abs %.3e, bar %.3e" % (what, err, bar)
        assert torch.equal(o1, o0), "%s: out differs from the general form, max |d| %.3e" % (what, (o1 - o0).abs().max().item())
        if y0 is not None:
            assert not torch.isnan(y1).any(), "%s: y not written completely" % what
            assert torch.equal(y1, y0), "%s: y differs from the general form" % what


SINGLE = {
    # name: (members, form)
    "straddle-relu": (lambda: [Member(2, 48, 48, 16, 12, "s1")], 1),                   # 3 fragments per crop: runs of 2 straddle the crops
    "straddle-res1": (lambda: [Member(2, 48, 48, 16, 12, "s2", res1=True)], 2),
    "two-blocks-res1": (lambda: [Member(2, 48, 96, 32, 24, "tb", res1=True)], 2),
    "nt4": (lambda: [Member(1, 64, 64, 16, 12, "n4")], 1),                             # conv_wino_f32<1, 4>
    "nt4-res1": (lambda: [Member(1, 64, 64, 16, 12, "n4r", res1=True)], 2),
    "ragged-res1": (lambda: [Member(1, 48, 48, 14, 10, "rg", res1=True)], 2),          # pixels outside the map: the out-of-range offset
    "fused-relu": (lambda: [Member(2, 48, 48, 32, 24, "f1", scales=(2, 4))], 1),       # conv_wino_fin_f32<1, 3>, terms at 1/2 and 1/4
    "fused-res1": (lambda: [Member(2, 48, 48, 32, 24, "f2", scales=(2, 4), res1=True)], 2),
    "no-relu": (lambda: [Member(2, 48, 48, 16, 12, "nr", relu=False)], 0),             # (the general form behind the same switch)
    "res-post": (lambda: [Member(2, 48, 48, 16, 12, "rp", res_post=True)], 0),
}


@pytest.mark.parametrize("seq", [1, 2])
@pytest.mark.parametrize("name", list(SINGLE))
def test_forms_match_float64_and_the_general_form_bitwise(name, seq):
    make, want = SINGLE[name]
    _both(name, make, want, seq=seq)


def _stage3(res1):
    return lambda: [Member(2, 48, 48, 32, 24, "g48", res1=res1), Member(2, 96, 96, 16, 12, "g96", res1=res1), Member(2, 192, 192, 8, 6, "g192", res1=res1)]


@pytest.mark.parametrize("table", [True, False], ids=["table", "banded"])
@pytest.mark.parametrize("res1", [False, True], ids=["form1", "form2"])
def test_grouped_stage3_launch_in_both_forms(res1, table):
    _both("stage3-%d" % res1, _stage3(res1), 2 if res1 else 1, seq=2 if table else 1, table=table)


@pytest.mark.parametrize("table", [True, False], ids=["table", "banded"])
def test_a_mixed_group_falls_back_to_the_general_form(table):
    make = lambda: [Member(2, 48, 48, 32, 24, "m48", res1=True), Member(2, 96, 96, 16, 12, "m96"), Member(2, 192, 192, 8, 6, "m192", res1=True)]
    _both("mixed", make, 0, table=table)


def _model(forms_on):
    saved = engine.WINO_FORMS
    engine.WINO_FORMS = forms_on
    try:
        from i2r_amd import arch, config
        cfg = config.load_config("w48_pure_en6")
        sd = synth.make_state_dict(arch.param_spec(cfg))
        x, m, length = synth.make_inputs([2, 2], 256, 192, seed=7)
        net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
        y = net(x.cuda(), m.cuda(), length).cpu()
        groups = [st for P, *_ in net.engine().programs.values() for k, _, st in P.ops if k == cabi.OP_CONV_GROUP and st.d[0].contents.algo == 1]
        return y, sorted({_form(st) for st in groups})
    finally:
        engine.WINO_FORMS = saved
        engine.push_wino_forms()


def test_model_heat_maps_are_bitwise_equal_with_and_without_forms():
    """vanilla config, 2 images x 2 persons: every Winograd launch of the tower takes form 1 or 2 with the switch on, form 0 with it off"""
    y0, f0 = _model(False)
    y1, f1 = _model(True)
    assert f0 == [0] and f1 == [1, 2], (f0, f1)
    assert torch.isfinite(y0).all() and torch.equal(y0, y1), "max |d| %.3e" % (y0 - y1).abs().max().item()
