"""-m gpu: the scheduled pass loop of the Winograd kernels (csrc/i2r_conv_wino.hip, WINO_PASS) at the smallest shapes where a schedule
can go wrong.  The pass comes in copies -- first + more chunks, middle, last, only -- so the cases walk cin = 16 (one pass: the `only`
copy), 32 (first + last: one buffer swap), 48 (first + middle + last); one and two channel blocks on <1, 3> (cout 48, 96) and <1, 4>
(cout 64); maps 16x12, 8x8 and a ragged 10x6 whose fragments hang over the map; 1 and 2 crops; the fused-input staging with one and with
two terms (y prefilled with NaN); bias + ReLU (form 1), bias + res1 + ReLU (form 2) and the general form with res_post.

Every case is launched with the general epilogue at one fragment per workgroup and checked against float64 at the bar of the existing
Winograd tests, 2e-5 of max |ref|; then with the compile-time forms on, and as runs of two and of three fragments (seq 2 / 3: a 16x12
map has three fragments per crop, so a run of two ends in an empty tail at one crop and straddles the crops at two), each bit for bit
against the first launch: those pairs share nothing but the pass loop."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from _gpu_util import from_act, run, to_act
from i2r_amd import cabi, engine, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(31, key, tuple(shape), scale))


class Member:
    """one conv with its float64 reference: input (plus up-sampled terms at 1 / scales: the fused-input form), folded BN, residual in
    front of the ReLU (res1) or behind it (res_post)"""

    def __init__(self, n, cin, cout, h, w, tag, scales=(), res1=False, res_post=False):
        self.scales, self.tag = scales, tag
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
        self.y_ref = F.relu(y) if scales else None
        y = self.y_ref if scales else y
        sd = {k: v.double() for k, v in self.sd.items()}
        ref = F.batch_norm(F.conv2d(y, sd["c.weight"], None, padding=1), sd["b.running_mean"], sd["b.running_var"], sd["b.weight"], sd["b.bias"], False, 0.0, 1e-5)
        if res1:
            ref = ref + self.res1.double()
        ref = F.relu(ref)
        if res_post:
            ref = ref + self.res_post.double()
        self.ref = ref

    def emit(self, P, grp):
        pc = engine.Packer(self.sd, torch.device(DEV)).conv("c", "b")
        base, terms = to_act(P, self.base), [to_act(P, t) for t in self.terms]
        kw = dict(relu=True, group=grp, res1=to_act(P, self.res1) if self.res1 is not None else None,
                  res_post=to_act(P, self.res_post) if self.res_post is not None else None)
        self.y = None
        if self.scales:
            self.y = P.alloc(base.n, base.h, base.w, base.c)
            self.y.t.fill_(NAN)
            kw["fuse_in"] = (terms, self.y)
        self.out = P.conv(base, pc, **kw)
        self.out.t.fill_(NAN)


def _launch(m, forms_on, seq):
    """-> (kernel name, form, y or None, out as stored, out NCHW float64) of one launch of the member"""
    saved = engine.WINO_FORMS
    engine.WINO_FORMS = forms_on
    try:
        P = engine.Program(torch.device(DEV))
        grp = []
        m.emit(P, grp)
        assert grp[0][0].algo == 1
        grp[0][0].seq = seq
        P.flush_group(grp)
        (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
        engine.push_wino_forms()
        arr = (C.POINTER(cabi.ConvDesc) * st.n)(*[st.d[i] for i in range(st.n)])
        form, name = C.c_int32(-1), C.create_string_buffer(96)
        cabi.check(cabi.lib().i2r_conv_wino_form(arr, st.n, C.byref(form)), "i2r_conv_wino_form")
        cabi.check(cabi.lib().i2r_conv_kernel_name(arr, st.n, name, 96), "i2r_conv_kernel_name")
        run(P)
        return name.value.decode(), form.value, (m.y.view().clone() if m.y is not None else None), m.out.view().clone(), from_act(m.out).double()
    finally:
        engine.WINO_FORMS = saved
        engine.push_wino_forms()


CASES = {
    # name: (member, kernel, form with the forms on)
    "only-pass-1-crop": (lambda: Member(1, 16, 48, 16, 12, "a"), "conv_wino_f32<1, 3", 1),                        # 3 fragments: seq 2 ends in an empty tail
    "only-pass-ragged-two-blocks": (lambda: Member(2, 16, 96, 10, 6, "b", res1=True), "conv_wino_f32<1, 3", 2),
    "two-passes-8x8": (lambda: Member(2, 32, 96, 8, 8, "c", res1=True), "conv_wino_f32<1, 3", 2),                 # 2 fragments: seq 3 ends in an empty tail
    "two-passes-nt4": (lambda: Member(1, 32, 64, 16, 12, "d"), "conv_wino_f32<1, 4", 1),
    "three-passes-ragged": (lambda: Member(2, 48, 48, 10, 6, "e"), "conv_wino_f32<1, 3", 1),
    "three-passes-straddle": (lambda: Member(2, 48, 96, 16, 12, "f", res1=True), "conv_wino_f32<1, 3", 2),        # 6 fragments: runs of 2 straddle the crops
    "three-passes-nt4-res1": (lambda: Member(2, 48, 64, 8, 8, "g", res1=True), "conv_wino_f32<1, 4", 2),
    "general-res-post": (lambda: Member(2, 48, 48, 8, 8, "h", res_post=True), "conv_wino_f32<1, 3", 0),
    "general-res-post-only-pass": (lambda: Member(1, 16, 48, 10, 6, "i", res_post=True), "conv_wino_f32<1, 3", 0),
    "fused-one-term-two-passes": (lambda: Member(1, 32, 48, 16, 12, "j", scales=(2,)), "conv_wino_fin_f32<1, 3", 1),
    "fused-two-terms-three-passes": (lambda: Member(2, 48, 96, 16, 12, "k", scales=(2, 4), res1=True), "conv_wino_fin_f32<1, 3", 2),
    "fused-two-terms-only-pass": (lambda: Member(2, 16, 48, 8, 8, "l", scales=(2, 4)), "conv_wino_fin_f32<1, 3", 1),
}
_BASE = {}  # case -> (member with its float64 reference, results of the general form at seq 1): computed once, never changed


def _base(name):
    if name not in _BASE:
        make, kernel, _ = CASES[name]
        m = make()
        got = _launch(m, False, 1)
        assert got[0].startswith(kernel) and got[1] == 0, got[:2]
        _BASE[name] = (m, got)
    return _BASE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_general_form_matches_float64(name):
    m, (kernel, _, y, o, o64) = _base(name)
    err, bar = (o64 - m.ref).abs().max().item(), 2e-5 * m.ref.abs().max().item()
    print("%s (%s): max |got - ref| %.3e (bar %.3e)" % (name, kernel, err, bar))
    assert not torch.isnan(o[..., :m.out.c]).any(), "out not written completely"
    assert err < bar, "%s: max-abs %.3e, bar %.3e" % (name, err, bar)
    if y is not None:  # the fused sum is written on the way, every pixel and channel once: exact in fp32 against float64 up to one rounding per add
        assert not torch.isnan(y).any(), "y not written completely"
        yerr = (y[..., :m.base.shape[1]].permute(0, 3, 1, 2).double().cpu() - m.y_ref).abs().max().item()
        ybar = 2e-5 * m.y_ref.abs().max().item()
        print("%s: y max |got - ref| %.3e (bar %.3e)" % (name, yerr, ybar))
        assert yerr < ybar


@pytest.mark.parametrize("how", ["forms", "seq2", "seq3", "forms-seq2"])
@pytest.mark.parametrize("name", list(CASES))
def test_forms_and_runs_match_the_general_form_bitwise(name, how):
    m, (kernel0, _, y0, o0, _) = _base(name)
    forms_on, seq = how.startswith("forms"), {"forms": 1, "seq2": 2, "seq3": 3, "forms-seq2": 2}[how]
    kernel, form, y1, o1, _ = _launch(m, forms_on, seq)
    assert kernel.startswith(CASES[name][1]) and form == (CASES[name][2] if forms_on else 0), (kernel, form)
    assert not torch.isnan(o1[..., :m.out.c]).any(), "out not written completely"
    assert torch.equal(o1, o0), "%s %s: out differs from %s at seq 1, max |d| %.3e" % (name, how, kernel0, (o1 - o0).abs().max().item())
    if y0 is not None:
        assert not torch.isnan(y1).any(), "y not written completely"
        assert torch.equal(y1, y0), "%s %s: y differs" % (name, how)
