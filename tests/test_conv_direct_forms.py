"""CPU: what a direct fp32 conv launch resolves to (i2r_conv_direct_form launches nothing) for the case table of _conv_direct_cases.py, the
process-wide switch (i2r_conv_direct_forms, engine.CONV_FORMS), and that both exports are additive: header, binding and library agree and
the ABI version and the kernel names are what they were."""
import ctypes as C
import os
import re

import pytest

import _conv_cases as cc
import _conv_direct_cases as dc
from i2r_amd import cabi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _switch_on():
    cabi.lib().i2r_conv_direct_forms(1)
    yield
    cabi.lib().i2r_conv_direct_forms(1)


@pytest.mark.parametrize("key", list(dc.SINGLES))
def test_single_launch_resolves_to_its_instantiation_and_form(key):
    c, name, want = dc.SINGLES[key]
    assert cc.resolve([c.desc()]) == (0, name, "")
    assert dc.direct_form([c.desc()]) == want


@pytest.mark.parametrize("key", list(dc.GROUPS))
def test_grouped_launch_resolves_to_its_instantiation_and_form(key):
    members, name, want = dc.GROUPS[key]
    descs = [m.desc() for m in members]
    assert cc.resolve(descs) == (0, name, "")
    assert dc.direct_form(descs) == want
    assert len({m.cin * len(m.taps) for m in members}) == 3, "three members with different K"


def test_the_table_reaches_every_body_and_epilogue_form_and_every_tail_of_the_k_loop():
    forms = {w for _, _, w in dc.SINGLES.values()} | {w for _, _, w in dc.GROUPS.values()}
    assert forms >= {(0, 0), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)}
    names = {n for c, n, w in dc.SINGLES.values() if w[0]}
    assert {re.match(r"conv_igemm_f32<(\d)", n).group(1) for n in names} == {"1", "2", "3"}
    assert {re.match(r"conv_igemm_f32<\d, (\d)", n).group(1) for n in names} == {"3", "4", "5"}
    assert {n[-7:] for n in names} == {" 12, 1>", ", 4, 1>", ", 4, 2>"}


def test_switch_off_means_the_general_body_everywhere_and_names_do_not_change():
    L = cabi.lib()
    before = {k: cc.resolve([c.desc()])[1] for k, (c, _, _) in dc.SINGLES.items()}
    assert L.i2r_conv_direct_forms(0) == 0
    for k, (c, name, _) in dc.SINGLES.items():
        assert dc.direct_form([c.desc()]) == (0, 0), k
        assert cc.resolve([c.desc()])[1] == before[k] == name
    for members, _, _ in dc.GROUPS.values():
        assert dc.direct_form([m.desc() for m in members]) == (0, 0)
    assert L.i2r_conv_direct_forms(1) == 0
    assert dc.direct_form([dc.SINGLES["single-res1"][0].desc()]) == (1, 2)


def test_four_m_fragments_16_bit_operands_and_winograd_report_form_0():
    mt4 = next(c for c in cc.CASES if c.dtype == 0 and c.mt == 4 and c.variant[1] > 0)
    assert dc.direct_form([mt4.desc()]) == (0, 0)
    lp = next(c for c in cc.CASES if c.dtype == 1 and c.variant[1] > 0)
    assert dc.direct_form([lp.desc()]) == (0, 0)
    d = dc.mk("w", cin=48, cout=48, k=3, s=1, conv=(16, 12), tile=(0, 0), mt=0, wn=0).desc()
    d.algo = 1
    assert dc.direct_form([d]) == (0, 0)


def test_epi_may_be_null_and_form_may_not():
    L = cabi.lib()
    d = dc.SINGLES["single-relu"][0].desc()
    arr = (C.POINTER(cabi.ConvDesc) * 1)(C.pointer(d))
    f = C.c_int32(-1)
    assert L.i2r_conv_direct_form(arr, 1, C.byref(f), None) == 0 and f.value == 1
    assert L.i2r_conv_direct_form(arr, 1, None, None) != 0


def test_exports_are_additive():
    hdr = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    for name in ("i2r_conv_direct_form", "i2r_conv_direct_forms"):
        assert name in cabi.EXPORTS and re.search(r"^I2R_API int %s\(" % name, hdr, flags=re.M)
        assert hasattr(cabi.lib(), name)
    assert cabi.lib().i2r_conv_direct_forms.argtypes == [C.c_int32]
    assert cabi.ABI_VERSION == 17 and cabi.lib().i2r_abi_version() == 17


def test_engine_switch_reaches_the_library():
    d = dc.SINGLES["single-res1"][0].desc()
    saved = engine.CONV_FORMS
    try:
        for on, want in ((False, (0, 0)), (True, (1, 2))):
            engine.CONV_FORMS = on
            engine.push_conv_forms()
            assert dc.direct_form([d]) == want
    finally:
        engine.CONV_FORMS = saved
        engine.push_conv_forms()
    assert engine.CONV_FORMS is True
