"""CPU: the case table of _mh_cases.py reaches every instantiation of enc_mh_attn_k<HB, NQ>, every workgroup shape and both sides of the
launcher's two breaks -- asked of the library through i2r_mh_attention_form, which launches nothing -- the loop reference is the oracle's
attention (and a padded, key_padding_mask-style restatement under key_len), fp32 restatements of every case stay within a quarter of the
tolerance against float64 (the tolerance is not what makes a case pass), wrong variants differ from the reference by 50 x the tolerance
in every case they apply to, and the new export is additive."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _mh_cases as mc
import i2r_cpu
from _encoder_cases import EDGE, counts
from i2r_amd import cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(mc.CASES)
MUTANT_MIN = 1e-3     # 50 x TOL


def _form(case):
    return mc.form(mc.args_for(case))


def test_edge_is_what_the_table_says():
    assert sum(EDGE) == 724 and counts(EDGE)[:3] == (53, 31, 19)
    assert mc.TOL == 2e-5 and MUTANT_MIN == 50 * mc.TOL
    assert len(mc.INSTANTIATIONS) == 24 == len(mc.NQ1_HB) + len(mc.NQ2_HB) + len(mc.NQ4_HB)


def test_the_table_reaches_all_24_instantiations():
    met = {}
    for name, case in mc.CASES.items():
        f = _form(case)
        assert f.hb == case.hp // 16 and f.nq == case.nq, "%s runs <%d,%d>" % (name, f.hb, f.nq)
        met.setdefault((f.hb, f.nq), []).append(name)
    print("MH-COVERAGE " + " ".join("<%d,%d>:%s" % (k + (",".join(v),)) for k, v in sorted(met.items())))
    assert set(met) == mc.INSTANTIATIONS
    # the edges that must meet the wider query tiles: stride gaps, key_len, rising keys and many short groups at NQ 1, 2 and 4
    for pick in (lambda c: c.gaps != (0, 0, 0, 0), lambda c: c.key_len == "cycle", lambda c: c.rising):
        assert {c.nq for c in mc.CASES.values() if pick(c)} == {1, 2, 4}
    many = mc.CASES["many-n4"]
    assert len(many.lens) == 320 and max(many.lens) < 64 and many.nq == 4
    assert mc.CASES["tail-rows"].tail == 37 and {c.name for c in mc.CASES.values() if c.tail} == {"tail-rows"}


def test_every_workgroup_shape_and_the_grid_of_every_case():
    shapes = {}
    for name, case in mc.CASES.items():
        f = _form(case)
        wpb, live = mc.block_shape(case.heads)
        tiles = counts(case.lens)[{1: 0, 2: 1, 4: 2}[f.nq]]
        assert f.grid == (tiles, -(-case.heads // wpb)) and f.block == 64 * wpb, name
        assert (f.grid[1] - 1) * wpb + live == case.heads and 1 <= live <= wpb
        shapes.setdefault((wpb, live), []).append(name)
    print("MH-SHAPES " + " ".join("wpb%d/last%d:%d" % (k + (len(v),)) for k, v in sorted(shapes.items())))
    # wpb = heads for 1, 2, 3 heads; full blocks of four; a last block with 1, 2 and 3 live waves
    assert set(shapes) == {(1, 1), (2, 2), (3, 3), (4, 4), (4, 1), (4, 2), (4, 3)}
    # each of the seven at NQ = 1 (every width's table entry carries one), the partial blocks also beside a full one
    assert {mc.block_shape(c.heads) for c in mc.CASES.values() if c.nq == 1 and c.name.startswith("w")} == set(shapes)
    assert {c.heads for c in mc.CASES.values() if c.name.startswith("w")} == {1, 2, 3, 4, 5, 6, 7, 8}


def test_each_threshold_case_sits_on_the_side_it_names():
    waves = lambda name, i: counts(mc.CASES[name].lens)[i] * mc.CASES[name].heads
    nq = lambda name: _form(mc.CASES[name]).nq
    assert waves("t4-4096", 2) == mc.MIN_WAVES and nq("t4-4096") == 4
    assert waves("t4-4095", 2) == mc.MIN_WAVES - 1 and nq("t4-4095") == 2 and waves("t4-4095", 1) >= mc.MIN_WAVES
    for w in ("", "-w48"):
        assert waves("t2-4096" + w, 1) == mc.MIN_WAVES and nq("t2-4096" + w) == 2
        assert waves("t2-4095" + w, 1) == mc.MIN_WAVES - 1 and nq("t2-4095" + w) == 1
    assert {mc.CASES[n].hp for n in ("t4-4096", "t4-4095")} == {32} and {mc.CASES["t2-4096" + w].hp for w in ("", "-w48")} == {96, 48}
    far = mc.CASES["far-w112"]
    assert waves("far-w112", 1) >= mc.MIN_WAVES and waves("far-w112", 0) == 7632 and far.hp // 16 == 7 and nq("far-w112") == 1
    # NQ = 2 at HB 1, 2: below the break in 64-query tiles, above it in 32-query tiles
    for n in ("n2-w16", "n2-w32"):
        assert waves(n, 2) < mc.MIN_WAVES <= waves(n, 1)
    # the same arguments one tile count apart, through the query alone
    a = mc.args_for(mc.CASES["t4-4096"])
    assert mc.form(a).nq == 4
    a.n_qtiles64 -= 1
    assert mc.form(a).nq == 2
    a = mc.args_for(mc.CASES["t2-4096"])
    a.n_qtiles32 -= 1
    a.n_qtiles64 -= 1
    assert mc.form(a).nq == 1


def test_stride_and_key_len_cases_hold_the_edges_they_name():
    st = [c for c in mc.CASES.values() if c.gaps != (0, 0, 0, 0)]
    assert {c.gaps[3] for c in st} == {4, 12, 20, 36} and {c.gaps[:3] for c in st} == {(8, 12, 4)}
    assert {c.heads for c in st} >= {1, 5}
    for c in st:
        hs, k_off, qk_cs, v_cs, out_cs = mc.strides(c)
        assert (k_off, qk_cs, v_cs) == (hs + 8, k_off + hs + 12, hs + 4) and out_cs - hs == c.gaps[3]
    # the pad fill of lane group g starts at column hs + 4 g and steps by 16: which lane groups store, and how many trips
    trips = {gap: [len(range(4 * g, gap, 16)) for g in range(4)] for gap in (4, 12, 20, 36)}
    assert trips == {4: [1, 0, 0, 0], 12: [1, 1, 1, 0], 20: [2, 1, 1, 1], 36: [3, 2, 2, 2]}
    # key_len: every pattern meets every EDGE length in kl-n1, all inside the precondition; the clamp case is outside it
    c = mc.CASES["kl-n1"]
    kl = mc.key_lens(c)
    assert {(mc.key_len_pattern(i, 6), n) for i, n in enumerate(c.lens)} == {(p, n) for p in range(6) for n in EDGE}
    assert all(1 <= k <= n for k, n in zip(kl, c.lens)) and mc.clamped(kl, c.lens) == kl
    assert any(k < n for k, n in zip(kl, c.lens)) and {16, 17} <= set(kl)
    c = mc.CASES["kl-clamp"]
    kl = mc.key_lens(c)
    assert {k for k in kl if k <= 0} == {0, -5} and any(k == n + 7 for k, n in zip(kl, c.lens))
    assert mc.clamped(kl, c.lens) == [1 if k <= 0 else n for k, n in zip(kl, c.lens)]
    assert {(mc.key_len_pattern(i, 3), n) for i, n in enumerate(c.lens)} == {(p, n) for p in range(3) for n in EDGE}


def test_inputs_are_what_the_module_says():
    for name in ("w16-h1", "w256-h7", "rise-n1"):
        case = mc.CASES[name]
        q, k, v = mc.inputs(name)
        assert q.shape == (sum(case.lens), case.heads, case.hp) and q.dtype == torch.float32
        assert all((t[..., case.hd:] == 0).all() for t in (q, k, v))
        assert v.abs().max().item() <= 1.0 and 0.9 < k[..., :case.hd].pow(2).mean().item() < 1.1
        assert abs(q[..., :case.hd].pow(2).mean().item() * case.hd / case.scale ** 2 - 1.0) < 0.1
    # rising: the scores of each group's first query grow key by key, in every head
    case = mc.CASES["rise-n1"]
    q, k, v = mc.inputs("rise-n1")
    g0 = 0
    for n in case.lens:
        s0 = torch.einsum("hd,khd->hk", q[g0].double(), k[g0:g0 + n].double())
        assert (s0[:, 1:] >= s0[:, :-1]).all()
        g0 += n


BAD = (dict(hp=12), dict(hp=272), dict(k_off=16), dict(qk_cs=48), dict(v_cs=16), dict(out_cs=30), dict(n_qtiles16=0), dict(n_qtiles64=0),
       dict(n_qtiles32=2), dict(heads=0), dict(qk=None))   # the list of test_kernels_gpu.py::test_mh_attention_rejects_bad_arguments


def test_the_query_rejects_what_a_launch_rejects_and_launches_nothing():
    L = cabi.lib()
    ok = dict(qk=0x1000, v=0x2000, out=0x3000, grp_off=0x4000, n_grp=1, heads=2, hp=16, k_off=32, qk_cs=64, v_cs=32, out_cs=32, n_qtiles16=1,
              n_qtiles32=1, n_qtiles64=1)
    hb, nq, block, grid = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), (C.c_int32 * 2)(-1, -1)
    a = cabi.MhAttnArgs(**ok)
    assert L.i2r_mh_attention_form(C.byref(a), C.byref(hb), C.byref(nq), grid, C.byref(block)) == 0      # (no device here: nothing ran)
    assert (hb.value, nq.value, grid[0], grid[1], block.value) == (1, 1, 1, 1, 128)
    assert L.i2r_mh_attention_form(C.byref(a), C.byref(hb), C.byref(nq), None, None) == 0
    assert L.i2r_mh_attention_form(C.byref(a), None, C.byref(nq), grid, C.byref(block)) != 0
    assert L.i2r_mh_attention_form(C.byref(a), C.byref(hb), None, grid, C.byref(block)) != 0 and b"i2r_mh_attention_form" in L.i2r_last_error()
    assert L.i2r_mh_attention_form(None, C.byref(hb), C.byref(nq), grid, C.byref(block)) != 0
    for bad in BAD:
        a = cabi.MhAttnArgs(**dict(ok, **bad))
        hb.value = nq.value = block.value = grid[0] = grid[1] = -1
        assert L.i2r_mh_attention_form(C.byref(a), C.byref(hb), C.byref(nq), grid, C.byref(block)) != 0, bad
        assert b"i2r_mh_attention" in L.i2r_last_error()
        assert (hb.value, nq.value, grid[0], grid[1], block.value) == (-1,) * 5, bad


def test_export_is_additive():
    hdr = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert "i2r_mh_attention_form" in cabi.EXPORTS and re.search(r"^I2R_API int i2r_mh_attention_form\(", hdr, flags=re.M)
    assert cabi.lib().i2r_mh_attention_form.argtypes == [C.POINTER(cabi.MhAttnArgs)] + [C.POINTER(C.c_int32)] * 4
    assert cabi.ABI_VERSION == 17 and cabi.lib().i2r_abi_version() == 17
    assert re.search(r"#define I2R_ABI_VERSION 17\b", hdr)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loop_reference_is_the_oracles_multi_head_attention_in_float64():
    """i2r_cpu.encoder_layer (pre-norm, n_head = 3) reduced to its attention: norm1 = 0 makes q and k projections of pos alone, an identity
    out-proj and a zero linear2 leave src + attention"""
    heads, hd = 3, 13
    d, n = heads * hd, sum(EDGE)
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    w, b, src, pos = rnd(3 * d, d) * d ** -0.5 * 2.0, rnd(3 * d) * 0.1, rnd(n, d), rnd(n, d)
    p = "E.layers.0"
    sd = {p + ".self_attn.in_proj_weight": w, p + ".self_attn.in_proj_bias": b,
          p + ".self_attn.out_proj.weight": torch.eye(d, dtype=torch.float64), p + ".self_attn.out_proj.bias": torch.zeros(d, dtype=torch.float64),
          p + ".norm1.weight": torch.zeros(d, dtype=torch.float64), p + ".norm1.bias": torch.zeros(d, dtype=torch.float64),
          p + ".norm2.weight": torch.ones(d, dtype=torch.float64), p + ".norm2.bias": torch.zeros(d, dtype=torch.float64),
          p + ".linear1.weight": rnd(2 * d, d), p + ".linear1.bias": rnd(2 * d),
          p + ".linear2.weight": torch.zeros(d, 2 * d, dtype=torch.float64), p + ".linear2.bias": torch.zeros(d, dtype=torch.float64)}
    out = i2r_cpu.inter_human_encoder(sd, "E", 1, src.reshape(n, d, 1, 1), pos.reshape(n, d, 1, 1), list(EDGE), n_head=heads, pre_norm=True)
    assert out.dtype == torch.float64
    att = out.reshape(n, d) - src
    q = ((pos @ w[:d].t() + b[:d]) * hd ** -0.5).reshape(n, heads, hd)
    k = (pos @ w[d:2 * d].t() + b[d:2 * d]).reshape(n, heads, hd)
    v = (src @ w[2 * d:].t() + b[2 * d:]).reshape(n, heads, hd)
    mine = mc.loop_reference(q, k, v, EDGE).reshape(n, d)
    assert att.abs().max().item() > 0.5 and (mine - att).abs().max().item() < 1e-12
    assert (mc.batched(q, k, v, EDGE) .reshape(n, d) - att).abs().max().item() < 1e-12


@pytest.mark.parametrize("name", ["kl-n1", "kl-clamp", "w48-h3"])
def test_loop_reference_equals_a_padded_and_masked_restatement(name):
    """groups padded to the longest one, the keys past the (clamped) key_len under a key_padding_mask, one batched softmax"""
    case = mc.CASES[name]
    q, k, v = (t.double() for t in mc.inputs(name))
    kl = mc.clamped(mc.key_lens(case), case.lens)
    G, N, H, hp = len(case.lens), max(case.lens), case.heads, case.hp
    Q, K, V = (torch.zeros(G, H, N, hp, dtype=torch.float64) for _ in range(3))
    mask = torch.ones(G, N, dtype=torch.bool)
    g0 = 0
    for i, n in enumerate(case.lens):
        for P, t in ((Q, q), (K, k), (V, v)):
            P[i, :, :n] = t[g0:g0 + n].transpose(0, 1)
        mask[i, :kl[i]] = False
        g0 += n
    O = torch.softmax((Q @ K.transpose(-1, -2)).masked_fill(mask[:, None, None, :], -math.inf), -1) @ V
    got = torch.cat([O[i, :, :n].transpose(0, 1) for i, n in enumerate(case.lens)])
    ref = mc.reference(name)
    assert (got[..., :case.hd] - ref).abs().max().item() < 1e-12
    # and the helpers the other checks stand on: the batched form and the tile-ordered form, both in float64
    assert (mc.batched(q, k, v, case.lens, mc.key_lens(case))[..., :case.hd] - ref).abs().max().item() < 1e-12
    assert (mc.online(q, k, v, case.lens, mc.key_lens(case), torch.float64)[..., :case.hd] - ref).abs().max().item() < 1e-12


@pytest.fixture(scope="module", params=NAMES)
def name(request):
    """module scope: pytest runs the tests of one case side by side, so its inputs and reference are made once"""
    return request.param


def test_tolerance_is_not_what_makes_a_case_pass(name):
    """plain fp32 torch, and fp32 in the kernel's order (exp2 domain, key tiles of 16, running rescale), against float64: within TOL / 4"""
    case = mc.CASES[name]
    q, k, v = mc.inputs(name)
    ref, kl = mc.reference(name), mc.key_lens(case)
    assert 0.3 < ref.abs().max().item() <= 1.0 and torch.isfinite(ref).all()      # |v| <= 1: the bar is absolute
    e_plain = (mc.batched(q, k, v, case.lens, kl, torch.float32)[..., :case.hd].double() - ref).abs().max().item()
    e_tiled = (mc.online(q, k, v, case.lens, kl)[..., :case.hd].double() - ref).abs().max().item()
    print("MH-FP32 %-12s plain %.2e = %.3f TOL  kernel order %.2e = %.3f TOL" % (name, e_plain, e_plain / mc.TOL, e_tiled, e_tiled / mc.TOL))
    assert max(e_plain, e_tiled) <= mc.TOL / 4


def test_wrong_variants_are_50_tolerances_away(name):
    case = mc.CASES[name]
    q, k, v = (t.double() for t in mc.inputs(name))
    ref, kl = mc.reference(name), mc.key_lens(case)
    for what, (fn, applies) in mc.MUTANTS.items():
        if applies(case):
            diff = (fn(case, q, k, v, kl)[..., :case.hd] - ref).abs().max().item()
            print("MH-MUTANT %-12s %-42s %.2e" % (name, what, diff))
            assert diff >= MUTANT_MIN, "%s: '%s' is only %.2e from the reference" % (name, what, diff)


def test_every_wrong_variant_applies_somewhere():
    for what, (_, applies) in mc.MUTANTS.items():
        assert any(applies(c) for c in mc.CASES.values()), what
    assert len(mc.MUTANTS) == 8
