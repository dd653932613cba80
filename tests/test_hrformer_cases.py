"""CPU side of the fp32 HRFormer-B cases (tests/_hrformer_cases.py): the loop-form window attention is the oracle's, every case's plain
fp32 torch restatement is well inside the case's tolerance against float64, and each table hits the edges it claims."""
import pytest
import torch

import _hrformer_cases as hc
import i2r_cpu_hrformer as H
from i2r_amd import arch

_ID = dict(ids=lambda c: c.id)


def _err(a, b):
    return (a.double() - b.double()).abs().max().item()


# ---- the loop form is the oracle's window attention ----
@pytest.mark.parametrize("c,heads,h,w", [(78, 2, 5, 9), (78, 2, 13, 3), (156, 4, 9, 8), (78, 2, 1, 2), (78, 2, 7, 7), (80, 2, 8, 15), (74, 2, 5, 9)])
def test_loop_form_window_attention_is_the_oracles(c, heads, h, w):
    """q / k / v projected with the oracle's weights into the kernel's layout, window_attention_loop, out_proj == oracle.window_attention
    in float64 to 1e-12 -- on maps whose padding is odd (5x9: 5 pad columns, 13x3: 1 pad row, 9x8: 5 pad rows), so the pad // 2-before
    convention is pinned by two independent statements of it"""
    spec = arch.Spec()
    p = "a"
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        spec.linear(p + "." + n, c, c)
    sd = {k: v.double() for k, v in hc.synth.make_state_dict(spec, seed=3).items()}
    x = hc.rand((2, h, w, c), "loop.x.%d.%d.%d" % (c, h, w)).double()
    ph, pw = -h % 7, -w % 7
    hd = c // heads
    qkv, bias = hc.project_qkv(sd, p, x, heads)
    a = hc.unpad_heads(hc.window_attention_loop(qkv, bias, heads, hd), heads, hd)
    got = torch.nn.functional.linear(a, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])
    ref = H.window_attention(sd, p, x, heads)
    assert got.shape == ref.shape
    assert _err(got, ref) < 1e-12, (ph, pw, _err(got, ref))


def test_loop_form_cases_include_odd_padding():
    odd = [(h, w) for h, w in [(5, 9), (13, 3), (9, 8)] if (-h % 7) % 2 == 1 or (-w % 7) % 2 == 1]
    assert len(odd) == 3


# ---- fp32 torch against float64: a quarter of the tolerance ----
@pytest.mark.parametrize("case", hc.LN_CASES, **_ID)
def test_layernorm_cases_are_well_conditioned(case):
    x, w, b = hc.ln_tensors(case)
    ref = hc.ln_ref(x.double(), w.double(), b.double())
    assert _err(hc.ln_fp32(x, w, b), ref) < 0.25 * hc.TOL_LN
    assert _err(ref, hc.ln_fp32(x.double(), w.double(), b.double())) < 1e-12   # the hand-written reference is torch's layer_norm
    assert 1.0 < ref.abs().max().item() < 4.0


@pytest.mark.parametrize("case", hc.WA_CASES, **_ID)
def test_window_attention_cases_are_well_conditioned(case):
    qkv, bias = hc.wa_tensors(case)
    ref = hc.window_attention_loop(qkv.double(), bias.double(), case.heads, case.hd)
    assert _err(hc.window_attention_loop(qkv, bias, case.heads, case.hd), ref) < 0.25 * hc.TOL_ATTN
    # the pad dims of q | k | v, of the bias vector and of the reference are exactly zero
    hs = case.heads * hc.HP
    for hh in range(case.heads):
        for t in (qkv[..., :hs], qkv[..., hs:2 * hs], qkv[..., 2 * hs:], ref):
            assert t[..., hh * hc.HP + case.hd:(hh + 1) * hc.HP].abs().sum().item() == 0.0
        assert all(bias[part * hs + hh * hc.HP + case.hd: part * hs + (hh + 1) * hc.HP].abs().sum().item() == 0.0 for part in range(3))


def test_window_attention_spread_case_reaches_its_scores():
    case = next(c for c in hc.WA_CASES if c.id.endswith("spread"))
    qkv, bias = hc.wa_tensors(case)
    hs = case.heads * hc.HP
    s = torch.einsum("nhwc,nhwc->nhw", qkv[..., :hc.HP].double(), qkv[..., hs:hs + hc.HP].double().roll(1, 2))
    assert 20.0 < s.abs().max().item() < 60.0


@pytest.mark.parametrize("case", hc.DW_CASES, **_ID)
def test_dwconv_cases_are_well_conditioned(case):
    x, sd = hc.dw_tensors(case)
    ref = hc.dw_ref(x.double(), sd, case.stride, case.act)
    assert _err(hc.dw_ref(x, sd, case.stride, case.act), ref) < 0.25 * hc.TOL_DW
    L = hc.dw_launch(case)
    assert tuple(ref.shape[2:]) == (L["out_h"], L["out_w"])


@pytest.mark.parametrize("case", hc.UP_CASES, **_ID)
def test_upsample_cases_are_well_conditioned(case):
    res, lows = hc.up_tensors(case)
    ref = hc.up_ref(res.double(), [t.double() for t in lows], case.scales, case.act)
    assert _err(hc.up_fp32(res, lows, case.scales, case.act), ref) < 0.25 * hc.up_tol(case)
    # the term-order reference is torch's bilinear interpolation
    assert _err(ref, hc.up_fp32(res.double(), [t.double() for t in lows], case.scales, case.act)) < 1e-12


@pytest.mark.parametrize("case", hc.BLOCK_CASES, **_ID)
def test_block_cases_are_well_conditioned(case):
    sd, st, x, ref, e32 = hc.block_reference(case)
    assert e32 < 0.25 * hc.TOL_BLOCK, e32
    assert 1.0 < ref.abs().max().item() < 6.0


@pytest.mark.parametrize("case", hc.MODULE_CASES, **_ID)
def test_module_cases_are_well_conditioned(case):
    sd, st, xs, refs, e32 = hc.module_reference(case)
    assert e32 < 0.25 * hc.TOL_MODULE, e32
    assert len(refs) == (case.nb if case.multiscale else 1)
    assert all(tuple(r.shape) == (case.n, hc._CH[i], case.h >> i, case.w >> i) for i, r in enumerate(refs))
    assert all(r.abs().max().item() > 0.5 for r in refs)


@pytest.mark.parametrize("case", hc.MODULE_CASES, **_ID)
def test_module_case_lane_schedules_have_no_race(case):
    """the lane program of every module case, built on the host as the GPU test builds it, replayed by the happens-before checker of
    tests/test_lanes.py: at these small maps the arena recycles buffers across shapes that never share an element count in the tower,
    and a hand-over that is too early need not show in the GPU test's results (its window is a few microseconds)"""
    from test_lanes import check_program
    from _gpu_util import to_act
    from i2r_amd import engine
    dev = torch.device("cpu")
    sd, st, xs, refs, e32 = hc.module_reference(case)
    pk = engine.Packer(sd, dev)
    mods = [engine.HRFormerB._module(pk, q, st, case.multiscale) for q in hc.module_keys(case.mods)]
    P = engine.Program(dev)
    ys = [to_act(P, x) for x in xs]
    mask = ((1 << case.nb) - 1) & ~1
    P.fork(mask)
    for mod in mods:
        ys = engine.HRFormerB._emit_module(P, mod, ys, True)
    P.join(mask)
    assert {lane for k, lane, _ in P.ops if k not in engine.cabi.SYNC_OPS} == set(range(case.nb))
    assert check_program(P) >= case.nb - 1   # (at least: the first output reads every other lane's branch)


# ---- every table hits the edges it claims ----
def test_case_ids_are_unique_and_every_case_names_its_edge():
    for table in hc.ALL_TABLES:
        ids = [c.id for c in table]
        assert len(set(ids)) == len(ids)
        assert all(len(c.edge) >= 6 for c in table)


def test_layernorm_table_hits_its_edges():
    L = {c.id: hc.ln_launch(c) for c in hc.LN_CASES}
    by = {c.id: c for c in hc.LN_CASES}
    assert sorted({c.c for c in hc.LN_CASES}) == [17, 78, 312, 624, 640]
    assert sorted({hc.ln_launch(c)["npix"] for c in hc.LN_CASES}) == [1, 15, 17, 3 * 9 * 7]
    assert len(L["c17"]["mixed"]) == 1 and len(L["c17"]["pad_chunks"]) >= 4   # one mixed chunk, whole pad chunks
    assert L["c78"]["mixed"] == [19] and L["c78"]["pad_chunks"] == []
    assert L["c624"]["cs"] == 624 and L["c640"]["cs"] == 640 and L["c640"]["nch"] == 160 == 16 * 10   # cs == c; the limit
    assert [L[i]["rounds"] for i in ("c17", "c78", "c312", "c624", "c640")] == [1, 2, 5, 10, 10]
    assert all((L[i]["cs"] // 4 > 16 * k) == (k < L[i]["rounds"]) for i in L for k in range(10))
    assert L["npix1"]["blocks"] == 1 and L["npix15"]["blocks"] == 1 and L["npix17"]["blocks"] == 2 and L["c78"]["blocks"] == 12
    assert L["c78"]["npix"] * 16 % 256 != 0   # a partial last workgroup
    assert by["shift8"].shift == 8.0
    assert {(c.c, c.out_dt) for c in hc.LN_CASES if c.out_dt} == {(78, 1), (78, 2), (624, 1), (624, 2)}


def test_window_attention_table_hits_its_edges():
    assert {(c.heads, c.hd) for c in hc.WA_CASES} == {(2, 39), (4, 39), (16, 39), (2, 40), (2, 37), (4, 38)}
    maps = {(c.h, c.w): hc.wa_launch(c) for c in hc.WA_CASES}
    assert {(7, 7), (1, 2), (5, 9), (13, 3), (8, 15), (14, 21)} <= set(maps)
    m = maps[(7, 7)]
    assert (m["nwy"], m["nwx"], m["pad_top"], m["pad_bottom"], m["pad_left"], m["pad_right"]) == (1, 1, 0, 0, 0, 0)
    m = maps[(1, 2)]
    assert (m["nwy"], m["nwx"], m["pad_top"], m["pad_bottom"], m["pad_left"], m["pad_right"]) == (1, 1, 3, 3, 2, 3)   # smaller than a window
    m = maps[(5, 9)]
    assert (m["nwy"], m["nwx"], m["pad_top"], m["pad_left"], m["pad_right"]) == (1, 2, 1, 2, 3)
    m = maps[(13, 3)]
    assert (m["nwy"], m["nwx"], m["pad_top"], m["pad_bottom"], m["pad_left"]) == (2, 1, 0, 1, 2)
    m = maps[(8, 15)]
    assert (m["nwy"], m["nwx"], m["pad_top"], m["pad_left"]) == (2, 3, 3, 3)
    m = maps[(14, 21)]
    assert (m["nwy"] * m["nwx"], m["pad_top"] + m["pad_bottom"] + m["pad_left"] + m["pad_right"]) == (6, 0)
    m = maps[(9, 8)]
    assert (m["pad_top"], m["pad_bottom"]) == (2, 3)
    for c in hc.WA_CASES:
        L = hc.wa_launch(c)
        assert 36 < c.hd <= 40 and L["hs"] == c.heads * 40 and L["c"] % c.heads == 0 and L["blocks"] > 1
    assert any(c.qscale > 1.0 for c in hc.WA_CASES)


def test_dwconv_table_hits_its_edges():
    s1 = [c for c in hc.DW_CASES if c.stride == 1]
    s2 = [c for c in hc.DW_CASES if c.stride == 2]
    assert {(c.h, c.w) for c in s1 if c.id.startswith("s1_") and c.id[3].isdigit()} == {(h, w) for h in (1, 2, 3, 5, 9) for w in (1, 7)}
    assert {hc.dw_launch(c)["strips"] for c in s1} == {1, 2, 3} and {hc.dw_launch(c)["tail_rows"] for c in s1} == {1, 2, 3}
    assert [hc.dw_launch(c)["strips"] for c in s1[:10:2]] == [(h + 3) // 4 for h in (1, 2, 3, 5, 9)]
    assert any(c.c == 1248 and hc.dw_launch(c)["cs"] == 1248 for c in s1) and any(hc.dw_launch(c)["cs"] > c.c for c in s1)
    assert {(c.act, c.bias, c.bn) for c in s1 if c.dt == 0} >= {(a, f, f) for a in (0, 1, 2) for f in (False, True)}
    assert {(c.dt, c.h) for c in s1 if c.dt} == {(1, 5), (1, 9), (2, 5), (2, 9)}
    assert {(c.c, c.h, c.w) for c in s2} == {(c, h, w) for c in (78, 156) for h, w in ((1, 1), (2, 3), (7, 5), (8, 6))}
    assert all(c.act == 0 and c.dt == 0 for c in s2)
    nthr = [hc.dw_launch(c)["nthr"] for c in hc.DW_CASES]
    assert any(n % 256 for n in nthr) and any(n < 256 for n in nthr) and any(n > 256 for n in nthr)   # partial, single and several workgroups


def test_upsample_table_hits_its_edges():
    one = [c for c in hc.UP_CASES if len(c.scales) == 1]
    assert {(c.scales[0], c.H // c.scales[0], c.W // c.scales[0]) for c in one} >= {(s, lh, lw) for s in (2, 4, 8) for lh, lw in ((1, 1), (1, 3), (3, 1), (3, 5))}
    multi = [c for c in hc.UP_CASES if len(c.scales) > 1]
    assert {c.scales for c in multi} == {(2, 2), (4, 2), (2, 4, 8), (8, 4, 2)} and all((c.H, c.W) == (16, 8) for c in multi)
    assert any((2, 1) in hc.up_launch(c)["lows"] for c in multi)   # the 1/8 map of 16x8 is 2x1
    assert {c.act for c in one} == {0, 1, 2} and {c.act for c in multi} == {0, 1, 2}
    assert any(c.alias for c in one) and any(c.alias for c in multi)
    assert all(c.H % s == 0 and c.W % s == 0 for c in hc.UP_CASES for s in c.scales)
    nthr = [hc.up_launch(c)["nthr"] for c in hc.UP_CASES]
    assert any(n % 256 for n in nthr) and any(n > 256 for n in nthr)


def test_block_and_module_tables_are_the_listed_ones():
    assert [(c.c, c.heads, c.h, c.w) for c in hc.BLOCK_CASES] == [(78, 2, 5, 9), (78, 2, 15, 8), (156, 4, 7, 7), (312, 8, 13, 3), (624, 16, 1, 2), (624, 16, 8, 6)]
    listed = [c for c in hc.MODULE_CASES if c.mods == 1]
    assert [(c.nb, c.h, c.w, c.blocks, c.multiscale) for c in listed] == [(2, 10, 6, 1, True), (3, 12, 20, 1, True), (4, 16, 8, 1, True),
                                                                         (4, 8, 16, 1, True), (4, 16, 8, 2, False)]
    assert [(c.nb, c.mods, c.multiscale) for c in hc.MODULE_CASES if c.mods > 1] == [(3, 2, True)]   # and a chain of two, as in a stage
    assert all(c.n == 2 for c in hc.MODULE_CASES)
    assert [(c.h >> 3, c.w >> 3) for c in hc.MODULE_CASES if c.nb == 4] == [(2, 1), (1, 2), (2, 1)]
    assert all(c.h % (1 << (c.nb - 1)) == 0 and c.w % (1 << (c.nb - 1)) == 0 for c in hc.MODULE_CASES)
