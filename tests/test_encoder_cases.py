"""CPU: the case table of _encoder_cases.py reaches every fp32 encoder layer instantiation and the edges of the launcher's rule -- asked of
the library through i2r_encoder_layer_form, which launches nothing -- its helpers are right (the fragment unpacking inverts
engine.pack_frag, the padded-and-masked float64 oracle equals a plain per-group loop, the reference magnitudes are the ones the bars of
test_encoder_fp32_gpu.py assume), and the new export is additive."""
import ctypes as C
import os
import re

import pytest
import torch

import _encoder_cases as ec
from i2r_amd import cabi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _form(case, d):
    return ec.layer_form(ec.dummy_desc(case.lens, d, scratch=case.scratch))


def test_edge_is_what_the_table_says():
    assert sum(ec.EDGE) == 724 and ec.counts(ec.EDGE)[:2] == (53, 31)
    assert min(ec.EDGE) == 1 and {n % 16 for n in ec.EDGE} >= {0, 1, 15}


@pytest.mark.parametrize("d", ec.DIMS)
def test_every_case_resolves_to_the_form_it_is_there_for(d):
    want = {"one-edge": (1, 1, 56), "one-many": (1, 1, 104), "one-big": (1, 1, 536), "split-edge": (1, 2, 512), "split-low": (1, 2, 512),
            "split-high": (1, 2, 512), "split-short": (1, 2, 512), "whole-noscratch": (1, 1, 320), "two-edge": (2, 1, 528),
            "two-threshold-512": (2, 1, 512), "two-threshold-511": (1, 1, 880), "tail-rows": (1, 1, 56)}
    assert set(want) == set(ec.CASES)
    for name, case in ec.CASES.items():
        assert _form(case, d) == want[name], name
    tiles = {n: ec.counts(c.lens) for n, c in ec.CASES.items()}
    assert tiles["one-many"][0] == 100 and len(ec.CASES["one-many"].lens) == 80
    assert tiles["one-big"][:2] == (530, 310)
    assert tiles["split-edge"][0] == tiles["whole-noscratch"][0] == 318
    assert tiles["split-low"][0] == 257 and tiles["split-high"][0] == 501 and tiles["split-short"][0] == 300
    assert tiles["two-edge"][1] == 527 and len(ec.CASES["two-edge"].lens) == 238
    assert tiles["two-threshold-512"][1] == 512 and tiles["two-threshold-511"][1] == 511


def test_the_table_reaches_all_six_instantiations_and_every_pos_mode_in_each():
    met = {}
    for name, d, nl in ec.VARIANTS:
        case = ec.CASES[name]
        qt, ks, _ = _form(case, d)
        met.setdefault((d, ec.FORM_NAMES[(qt, ks)]), set()).add(ec.pos_mode(case, d, nl))
    assert set(met) == {(d, f) for d in ec.DIMS for f in ("one", "split", "two")}
    assert all(m == set(ec.POS_MODES) for m in met.values()), met
    # single layer (no fused tail) and the three-layer stack both reach every form
    assert {nl for _, _, nl in ec.VARIANTS} == {1, 3}
    # the input shift is on half of the cases
    assert sum(c.shift for c in ec.CASES.values()) * 2 == len(ec.CASES)


@pytest.mark.parametrize("d", ec.DIMS)
def test_the_ends_of_the_split_range_and_the_two_tile_threshold(d):
    f = lambda lens, **kw: ec.layer_form(ec.dummy_desc(lens, d, **kw))
    assert f([16] * 256) == (1, 1, 256) and f([16] * 257) == (1, 2, 512)        # t_x 32 | 33
    assert f([16] * 504) == (1, 2, 512) and f([16] * 505) == (1, 1, 512)        # t_x 63 | 64
    assert f([16] * 497)[:2] == (1, 2)                                          # t_x 63 from its first tile count on
    assert f([16] * 300, scratch=False) == (1, 1, 304)                          # no scratch: one workgroup per tile
    assert f([32] * 511) == (1, 1, 1024) and f([32] * 512) == (2, 1, 512)       # 511 | 512 two-tile work items
    d1 = ec.dummy_desc([16] * 300, d)
    d1.split_cnt = None                                                         # half a scratch pair is no scratch
    assert ec.layer_form(d1) == (1, 1, 304)


def test_16_bit_selection_follows_the_documented_thresholds():
    for dtype in (1, 2):
        f = lambda lens, n192=None: ec.layer_form(_lp(lens, dtype, n192))
        assert f([64] * 511) == (1, 1, 4 * 511 + 4)         # n_qtiles64 = 511: 16 queries per wave, one item per 16-query tile
        assert f([64] * 512) == (12, 1, 512)                # n_qtiles64 = 512, n_qtiles192 = 512: four waves share 192 queries
        assert f([64] * 512, n192=0) == (4, 1, 512)         # n_qtiles192 = 0: 64 queries per wave
        assert f([768] * 43) == (12, 1, 176)                # 516 64-query tiles, 172 192-query items
        assert f([5] * 300) == (1, 1, 304)


def _lp(lens, dtype, n192):
    desc = ec.dummy_desc(lens, 96, dtype=dtype)
    if n192 is not None:
        desc.n_qtiles192 = n192
    return desc


def test_the_query_rejects_what_a_launch_rejects_and_null_form_pointers():
    L = cabi.lib()
    qt, ks, grid = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    ok = ec.dummy_desc(ec.EDGE)
    assert L.i2r_encoder_layer_form(C.byref(ok), C.byref(qt), C.byref(ks), None) == 0 and (qt.value, ks.value) == (1, 1)
    assert L.i2r_encoder_layer_form(C.byref(ok), None, C.byref(ks), C.byref(grid)) != 0
    assert L.i2r_encoder_layer_form(C.byref(ok), C.byref(qt), None, C.byref(grid)) != 0 and b"i2r_encoder_layer_form" in L.i2r_last_error()
    assert L.i2r_encoder_layer_form(None, C.byref(qt), C.byref(ks), C.byref(grid)) != 0
    for bad in (dict(cs=64), dict(dff_pad=96), dict(out=ok.src), dict(n_qtiles16=0), dict(n_qtiles32=0), dict(w2=None), dict(dtype=3),
                dict(next_w_in=0x10, next_b_in=0x20, next_kbuf=ok.kbuf, next_vbuf=0x30)):
        desc = ec.dummy_desc(ec.EDGE)
        for k, v in bad.items():
            setattr(desc, k, v)
        qt.value = ks.value = grid.value = -1
        assert L.i2r_encoder_layer_form(C.byref(desc), C.byref(qt), C.byref(ks), C.byref(grid)) != 0, bad
        assert (qt.value, ks.value, grid.value) == (-1, -1, -1) and b"i2r_encoder" in L.i2r_last_error()


def test_export_is_additive():
    hdr = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert "i2r_encoder_layer_form" in cabi.EXPORTS and re.search(r"^I2R_API int i2r_encoder_layer_form\(", hdr, flags=re.M)
    assert hasattr(cabi.lib(), "i2r_encoder_layer_form")
    assert cabi.lib().i2r_encoder_layer_form.argtypes == [C.POINTER(cabi.EncoderDesc)] + [C.POINTER(C.c_int32)] * 3
    assert cabi.ABI_VERSION == 17 and cabi.lib().i2r_abi_version() == 17
    assert re.search(r"#define I2R_ABI_VERSION 17\b", hdr)


@pytest.mark.parametrize("cs", (96, 80))
def test_unpack_kv_inverts_pack_frag(cs):
    n_frag = 5
    g = torch.Generator().manual_seed(cs)
    k = torch.randn(n_frag * 16, cs, generator=g)
    assert torch.equal(ec.unpack_kv(engine.pack_frag(k).reshape(-1), n_frag, cs), k.view(n_frag, 16, cs))
    v = torch.randn(n_frag, 16, cs, generator=g)                                 # [frag, key, dim]; the image is of V^T [dims, 16 keys]
    image = torch.cat([engine.pack_frag(v[f].t().contiguous()).reshape(-1) for f in range(n_frag)] + [torch.full((64,), 9.0)])
    assert torch.equal(ec.unpack_kv(image, n_frag, cs, vt=True), v)
    # element [frag f][dim 16 nt + li][key 4 g + r] sits where store_kv_frag puts it
    f, nt, li, gg, r = 3, 2, 7, 1, 2
    assert image[((f * (cs // 16) + nt) * 64 + 16 * gg + li) * 4 + r] == v[f, 4 * gg + r, 16 * nt + li]


def test_key_slots_number_fragments_group_by_group():
    frag, row, n = ec.key_slots([1, 17, 16, 33])
    assert n == 1 + 2 + 1 + 3
    assert frag.tolist()[:19] == [0] + [1] * 16 + [2, 3] and row.tolist()[:19] == [0] + list(range(16)) + [0, 0]
    assert frag[-1] == 6 and row[-1] == 0
    assert ec.kv_floats(724 + 37, 14, 96) == (47 + 14) * 16 * 96 >= ec.counts(ec.EDGE)[0] * 16 * 96


@pytest.mark.parametrize("d,mode_layers,want", [(96, 3, "none"), (78, 3, "rows"), (78, 1, "table")])
def test_masked_oracle_equals_a_plain_per_group_loop_in_float64(d, mode_layers, want):
    """the ragged case one-edge under each pos mode (see pos_mode for which run of the case has which)"""
    src, pos, _, mode = ec.inputs("one-edge", d, mode_layers)
    assert mode == want
    x = src.double()
    for i in range(3):
        a, b = ec.ref_layer(d, i, x, pos, ec.EDGE), ec.plain_layer(d, i, x, pos, ec.EDGE)
        assert a.dtype == torch.float64 and (a - b).abs().max().item() < 1e-12
        x = a
    stack = ec.ref_stack(d, 3, src, pos, ec.EDGE)
    assert (stack[-1] - x).abs().max().item() < 1e-12


def test_table_mode_is_token_modulo_period():
    src, pos, table, mode = ec.inputs("one-big", 96, 3)
    assert mode == "table" and table.shape == (ec.PERIOD, 96) and ec.PERIOD == 48
    assert torch.equal(pos[48 * 3 + 5], table[5]) and pos.shape == src.shape


@pytest.mark.parametrize("name,d,nl", [("one-edge", 96, 3), ("one-many", 78, 3), ("split-short", 96, 1), ("tail-rows", 78, 3), ("split-edge", 96, 3)])
def test_reference_magnitudes_stay_where_the_bars_assume_them(name, d, nl):
    """the absolute bars of the GPU module (4 x / 3 x the fp32 oracle's own error, max capped at 2e-4) presume outputs of a few units"""
    case = ec.CASES[name]
    src, pos, _, _ = ec.inputs(name, d, nl)
    outs = ec.ref_stack(d, nl, src, pos, case.lens)
    for o in outs:
        assert o.abs().max().item() < 8.0 and 0.5 < o.pow(2).mean().sqrt().item() < 2.0
    e_max, e_rms = ec.err_max_rms(ec.ref_layer(d, 0, src, pos, case.lens, torch.float32), outs[0])
    assert 0 < e_rms < e_max < 5e-5      # the fp32 oracle's own error on one layer: the unit the kernel's bar is counted in
