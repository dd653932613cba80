"""CPU: the epilogue form a Winograd launch resolves to (i2r_conv_wino_form launches nothing; csrc/i2r_conv_plan.h wino_form), the switch that
forces the general form (i2r_conv_wino_forms, engine.WINO_FORMS), and that both exports are additive: header, binding and library agree,
the ABI stays 17 and i2r_conv_desc still ends with seq."""
import ctypes as C
import os
import re

import pytest

import _conv_cases as cc
from i2r_amd import cabi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = [(t // 3, t % 3) for t in range(9)]


def wino_desc(n, c, h, w, cout=None, cout_pad=None, out_cs=None, relu=1, out=0x40000, **ptrs):
    cout = cout or c
    cout_pad = cout_pad or cout
    fw, fh = engine.wino_fragment(h, w)
    return cc.make_desc(n_img=n, in_h=h, in_w=w, in_cs=c, cin=c, conv_h=h, conv_w=w, out_h=h, out_w=w, out_cs=out_cs or cout_pad, cout=cout,
                        cout_pad=cout_pad, stride=1, iy0=-1, ix0=-1, taps=TAPS, tile_h=fh, tile_w=fw, mt=1, wn=1, relu=relu, algo=1, out=out, **ptrs)


def form(descs):
    arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
    f = C.c_int32(-1)
    cabi.check(cabi.lib().i2r_conv_wino_form(arr, len(descs), C.byref(f)), "i2r_conv_wino_form")
    return f.value


@pytest.fixture(autouse=True)
def _forms_on():
    cabi.lib().i2r_conv_wino_forms(1)
    yield
    cabi.lib().i2r_conv_wino_forms(1)


def test_lone_conv_with_relu_is_form_1_and_with_res1_form_2():
    assert form([wino_desc(2, 48, 16, 12)]) == 1
    assert form([wino_desc(2, 48, 16, 12, res1=0x60000)]) == 2
    assert form([wino_desc(1, 64, 16, 12)]) == 1                      # NT = 4
    assert form([wino_desc(2, 48, 32, 24, cout=96, res1=0x60000)]) == 2  # two channel blocks
    assert form([wino_desc(2, 48, 16, 12, out_cs=64)]) == 1           # (a wider row is no tail: every block is whole in cout and out_cs)


@pytest.mark.parametrize("what, kw", [("no-relu", dict(relu=0)), ("res2", dict(res1=0x60000, res2=0x70000)), ("res2-alone", dict(res2=0x70000)),
                                      ("res-post", dict(res_post=0x80000)), ("tail-40-of-48", dict(cout=40, cout_pad=48)),
                                      ("row-ends-in-the-block", dict(cout=40, cout_pad=48, out_cs=40))])
def test_everything_else_runs_the_general_form(what, kw):
    assert form([wino_desc(2, 48, 16, 12, **kw)]) == 0


def test_groups_take_a_form_only_when_every_member_agrees():
    a = lambda **kw: wino_desc(2, 192, 8, 6, out=0x40000, **kw)
    b = lambda **kw: wino_desc(2, 96, 16, 12, out=0x50000, **kw)
    c = lambda **kw: wino_desc(2, 48, 32, 24, out=0x60000, **kw)
    assert form([a(), b(), c()]) == 1
    assert form([a(res1=0x70000), b(res1=0x71000), c(res1=0x72000)]) == 2
    assert form([a(res1=0x70000), b(), c(res1=0x72000)]) == 0  # the members disagree on res1
    assert form([a(), b(res1=0x71000)]) == 0
    assert form([a(), b(relu=0), c()]) == 0
    assert form([a(res1=0x70000), b(res1=0x71000), c(res1=0x72000, res_post=0x73000)]) == 0


def test_the_switch_forces_the_general_form_and_comes_back():
    ds = [wino_desc(2, 48, 16, 12, res1=0x60000)]
    assert form(ds) == 2
    assert cabi.lib().i2r_conv_wino_forms(0) == 0
    assert form(ds) == 0 and form([wino_desc(2, 48, 16, 12)]) == 0
    assert cabi.lib().i2r_conv_wino_forms(1) == 0
    assert form(ds) == 2


def test_other_algorithms_report_form_0_and_the_kernel_name_does_not_carry_the_form():
    d = wino_desc(2, 48, 16, 12)
    assert cc.resolve([d]) == (0, "conv_wino_f32<1, 3>", "")
    assert cc.resolve([wino_desc(2, 48, 16, 12, res1=0x60000)]) == (0, "conv_wino_f32<1, 3>", "")
    d.algo, d.tile_h, d.tile_w, d.mt = 0, 0, 0, 0
    assert form([d]) == 0
    assert cabi.lib().i2r_conv_wino_form(None, 1, None) != 0  # (refused, not dereferenced)


def test_header_binding_and_exports_agree_and_the_abi_is_still_17():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    for name in ("i2r_conv_wino_form", "i2r_conv_wino_forms"):
        assert re.search(r"^I2R_API int %s\(" % name, header, flags=re.M) and name in cabi.EXPORTS
        assert getattr(cabi.lib(), name).restype is C.c_int
    assert cabi.lib().i2r_conv_wino_form.argtypes == [C.POINTER(C.POINTER(cabi.ConvDesc)), C.c_int32, C.POINTER(C.c_int32)]
    assert cabi.lib().i2r_conv_wino_forms.argtypes == [C.c_int32]
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION == cabi.lib().i2r_abi_version()
    assert cabi.ConvDesc._fields_[-1][0] == "seq"
    assert re.search(r"int32_t seq;[^}]*\} i2r_conv_desc;", header, flags=re.S)


def test_engine_constant_reaches_the_library():
    import torch
    from i2r_amd import synth
    sd = {"c.weight": torch.from_numpy(synth._sym(1, "w", (48, 48, 3, 3), 0.05))}
    pc = engine.Packer(sd, torch.device("cpu")).conv("c", None)
    saved = engine.WINO_FORMS
    try:
        for on in (False, True):
            engine.WINO_FORMS = on
            P = engine.Program(torch.device("cpu"))
            P.conv(P.alloc(2, 16, 12, 48), pc, relu=True)
            (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
            assert st.d[0].contents.algo == 1
            assert form([st.d[0].contents]) == (1 if on else 0)
    finally:
        engine.WINO_FORMS = saved
        engine.push_wino_forms()
