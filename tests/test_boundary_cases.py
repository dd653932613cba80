"""CPU: the float64 references of tests/_boundary_cases.py checked against themselves -- each restated a second way, a deliberately
wrong variant of every family rejected by the bound with a factor of 10 to spare, every kernel instantiation covered by a case, and
the inputs instructive (no case with more than 5 % of its elements bounded below 1e-6 of the map's largest value)."""
import pytest
import torch
import torch.nn.functional as F

import _boundary_cases as bc

REJECT = 10.0   # a wrong variant must exceed the bound by at least this factor somewhere


def _worst(wrong, ref, bound):
    return ((wrong - ref).abs() / bound).max().item()


# ---- the references restated ----
@pytest.mark.parametrize("cid", bc.ids(bc.STEM_CASES))
def test_stem_reference_is_the_tap_loop(cid):
    c = bc.BY_ID[cid]
    x, w, b = [t.double() for t in bc.stem_tensors(cid)]
    xs = bc.select(x, c.n, c.n_src, c.n_valid)
    oh, ow = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    xp = torch.zeros(c.n, c.cin, 2 * oh + 1, 2 * ow + 1, dtype=torch.float64)    # row / column 0 = image coordinate -1
    xp[:, :, 1:1 + c.h, 1:1 + c.w] = xs
    acc = b.view(1, 1, 1, -1).repeat(c.n, oh, ow, 1)
    mag = b.abs().view(1, 1, 1, -1).repeat(c.n, oh, ow, 1)
    for ky in range(3):
        for kx in range(3):
            for ci in range(c.cin):
                tap = xp[:, ci, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2].unsqueeze(-1)     # in[2 oy - 1 + ky][2 ox - 1 + kx]
                acc += tap * w[:, ci, ky, kx]
                mag += tap.abs() * w[:, ci, ky, kx].abs()
    ref, S = bc.stem_reference(cid)
    assert ref.shape == (c.n, oh, ow, c.cout)
    assert (ref - acc.clamp_min(0)).abs().max().item() <= 1e-13 and (S - mag).abs().max().item() <= 1e-13


@pytest.mark.parametrize("cid", bc.ids(bc.PE_RES_CASES))
def test_pe_res_reference_is_two_padded_convs(cid):
    c = bc.BY_ID[cid]
    m, w_pre, w7, b = [t.double() for t in bc.pe_res_tensors(cid)]
    ms = bc.select(m, c.n, c.n_src, c.n_valid)
    pre = F.conv2d(F.pad(ms, (1, 1, 1, 1)), w_pre)                       # [n, 3, h, w]: conv_pre's output, nothing outside the image
    out = F.relu(F.conv2d(F.pad(pre, (3, 3, 3, 3)), w7, b, stride=2))    # conv1 pads THAT with zeros
    ref, bound = bc.pe_res_reference(cid)
    assert ref.shape == (c.n, (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1, 64)
    assert (ref - out.permute(0, 2, 3, 1)).abs().max().item() <= 1e-13
    assert (bound > 0).all()


@pytest.mark.parametrize("cid", bc.ids(bc.CAT_CASES))
def test_cat_vec_reference_is_the_clipped_window_max(cid):
    """r cascaded MaxPool2d(3, 2, 1) = one max over [i 2^r - (2^r - 1), i 2^r + (2^r - 1)] clipped to the image"""
    c = bc.BY_ID[cid]
    m, wfc, bfc = bc.cat_tensors(cid)
    ms = bc.select(m, c.n, c.n_src, c.n_valid).double()
    R = (1 << c.rate) - 1
    assert ((c.h - 1) >> c.rate) + 1 == c.th and ((c.w - 1) >> c.rate) + 1 == c.tw
    pooled = torch.empty(c.n, c.th, c.tw, dtype=torch.float64)
    for iy in range(c.th):
        for ix in range(c.tw):
            y0, y1 = max((iy << c.rate) - R, 0), min((iy << c.rate) + R, c.h - 1)
            x0, x1 = max((ix << c.rate) - R, 0), min((ix << c.rate) + R, c.w - 1)
            pooled[:, iy, ix] = ms[:, y0:y1 + 1, x0:x1 + 1].amax((1, 2))
    assert torch.equal(pooled.flatten(1), bc.cat_pooled(ms, c.rate))
    if c.th > 1 and (ms < 0).all():
        assert (pooled[:, 0] != pooled[:, 1]).all(1).all(), "neighbouring windows with the same maximum"
    v, S = bc.cat_reference(cid)
    assert v.shape == (c.n, c.vec)
    loop = torch.stack([bfc.double() + sum(wfc[:, p].double() * pooled.flatten(1)[i, p] for p in range(c.th * c.tw)) for i in range(c.n)])
    assert (v - loop).abs().max().item() <= 1e-13


@pytest.mark.parametrize("cid", bc.ids(bc.POOL_CASES))
def test_pool_reference_is_the_window_loop(cid):
    c = bc.BY_ID[cid]
    x = bc.pool_tensors(cid).double()
    ref = bc.pool_reference(cid)
    oh, ow = (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1
    assert ref.shape == (c.n, oh, ow, c.c)
    for oy in range(oh):
        for ox in range(ow):
            win = x[:, max(2 * oy - 1, 0):min(2 * oy + 1, c.h - 1) + 1, max(2 * ox - 1, 0):min(2 * ox + 1, c.w - 1) + 1]
            assert torch.equal(ref[:, oy, ox], win.amax((1, 2)))
    assert torch.equal(ref.float().double(), ref)


@pytest.mark.parametrize("cid", bc.ids(bc.DECONV_CASES))
def test_deconv_reference_is_the_parity_tap_formula(cid):
    c = bc.BY_ID[cid]
    x, sd, _ = bc.deconv_tensors(cid)
    w, b = bc.deconv_folded(sd)
    ref, _ = bc.deconv_reference(cid, False, False)
    assert ref.shape == (c.n, c.cout, 2 * c.h, 2 * c.w)
    assert (ref - bc.deconv_by_parity(x, w, b, c.k)).abs().max().item() <= 1e-12
    # and the fold is the layer: BatchNorm applied to the unfolded transposed conv
    p, op = bc.DECONV_CFG[c.k]
    y = F.conv_transpose2d(x.double(), sd["d.weight"].double(), None, 2, p, op)
    y = F.batch_norm(y, sd["b.running_mean"].double(), sd["b.running_var"].double(), sd["b.weight"].double(), sd["b.bias"].double(), False, 0.0, 1e-5)
    assert (ref - y).abs().max().item() <= 1e-12


def test_fuse_reference_matches_float64_where_no_rounding_is_lost():
    """the fp32 sum of the reference against the float64 sum: equal after one rounding to fp32 wherever the float64 sum of the first
    two operands is itself an fp32 number (then nothing was rounded twice); and nearest up-sampling is F.interpolate's"""
    for c in bc.FUSE_CASES:
        base, terms = bc.fuse_tensors(c.id)
        for s, t in zip(c.scales, terms):
            assert torch.equal(bc.up_nearest(t.float(), s), F.interpolate(t.float().permute(0, 3, 1, 2), scale_factor=s, mode="nearest").permute(0, 2, 3, 1))
        ups = [bc.up_nearest(t.double(), s) for t, s in zip(terms, c.scales)]
        first = base.double() + ups[0]
        exact = first.float().double() == first
        total = first.float().double() + (ups[1] if len(ups) > 1 else 0.0)
        got = bc.fuse_value(base, terms, c.scales, 0, 0)
        assert exact.float().mean().item() > (0.2 if c.dt else 0.01)
        assert torch.equal(got.double()[exact], total.float().double()[exact])


# ---- deliberately wrong variants ----
@pytest.mark.parametrize("cid", [c.id for c in bc.STEM_CASES if c.n > c.n_src])
def test_stem_bound_rejects_a_mirrored_output(cid):
    """the mirror belongs to the INPUT: convolving the plain crop and mirroring the result differs (stride 2 on an even width reads
    other columns; the filter is not symmetric)"""
    c = bc.BY_ID[cid]
    x, w, b = bc.stem_tensors(cid)
    ref, S = bc.stem_reference(cid)
    plain, _ = bc.stem_value(bc.select(x, c.n_src, c.n_src, c.n_valid), w, b)
    wrong = torch.cat([plain, plain.flip(2)])
    assert _worst(wrong, ref, bc.fp32_bound(c.K, S)) >= REJECT


@pytest.mark.parametrize("cid", [c.id for c in bc.PE_RES_CASES if (c.h, c.w) != (1, 1)])
def test_pe_res_bound_rejects_an_unpadded_conv_pre(cid):
    """conv_pre evaluated outside the image too (the two convs merged into one 9x9 filter) instead of zeros around its output"""
    c = bc.BY_ID[cid]
    m, w_pre, w7, b = [t.double() for t in bc.pe_res_tensors(cid)]
    ms = bc.select(m, c.n, c.n_src, c.n_valid)
    wrong = F.relu(F.conv2d(F.conv2d(F.pad(ms, (4, 4, 4, 4)), w_pre), w7, b, stride=2)).permute(0, 2, 3, 1)
    ref, bound = bc.pe_res_reference(cid)
    assert wrong.shape == ref.shape and _worst(wrong, ref, bound) >= REJECT


@pytest.mark.parametrize("cid", [c.id for c in bc.PE_RES_CASES if c.n > c.n_src])
def test_pe_res_bound_rejects_a_mirrored_output(cid):
    c = bc.BY_ID[cid]
    m, w_pre, w7, b = bc.pe_res_tensors(cid)
    ref, bound = bc.pe_res_reference(cid)
    plain, _ = bc.pe_res_value(bc.select(m, c.n_src, c.n_src, c.n_valid), w_pre, w7, b)
    if (c.h, c.w) == (1, 1):
        assert torch.equal(torch.cat([plain, plain.flip(2)]), ref)   # (one pixel: nothing to mirror)
    else:
        assert _worst(torch.cat([plain, plain.flip(2)]), ref, bound) >= REJECT


@pytest.mark.parametrize("cid", bc.ids(bc.POOL_CASES))
def test_pool_reference_rejects_zero_padding(cid):
    """every case has windows that reach over the border and hold only negative elements: zero padding wins there, -inf does not"""
    ref, wrong = bc.pool_reference(cid), bc.pool_value(bc.pool_tensors(cid), 0.0)
    differ = ref != wrong
    border = torch.zeros_like(differ)
    border[:, 0], border[:, :, 0] = True, True        # windows of row 0 / column 0 always reach over the border
    assert differ[border].float().mean().item() > 0.25 and (wrong[differ] == 0).all()


@pytest.mark.parametrize("cid", [c.id for c in bc.CAT_CASES if c.rate > 0])
def test_cat_vec_bound_rejects_zero_padding_and_a_mirrored_output(cid):
    c = bc.BY_ID[cid]
    m, wfc, bfc = bc.cat_tensors(cid)
    ms = bc.select(m, c.n, c.n_src, c.n_valid)
    v, S = bc.cat_reference(cid)
    wrong, _ = bc.cat_value(bc.cat_pooled(ms, c.rate, 0.0), wfc, bfc)
    assert _worst(wrong, v, bc.fp32_bound(c.K, S)) >= REJECT
    if c.tw > 1:   # mirror applied to the pooled map instead of the mask
        plain = bc.cat_pooled(bc.select(m, c.n_src, c.n_src, c.n_valid), c.rate).view(c.n_src, c.th, c.tw)
        wrong, _ = bc.cat_value(torch.cat([plain, plain.flip(2)]).flatten(1), wfc, bfc)
        assert _worst(wrong, v, bc.fp32_bound(c.K, S)) >= REJECT


@pytest.mark.parametrize("cid", bc.ids(bc.HEAD_CASES))
def test_head_bound_rejects_a_dropped_channel_quadruple(cid):
    """the channel loop one quadruple short (the quad lanes' uneven shares)"""
    c = bc.BY_ID[cid]
    x, w, b = bc.head_tensors(cid)
    ref, S = bc.head_reference(cid)
    wrong, _ = bc.head_value(x[..., :c.cin - 4], w[:, :c.cin - 4], b)
    assert _worst(wrong, ref, bc.fp32_bound(c.K, S)) >= REJECT


@pytest.mark.parametrize("cid", bc.ids(bc.DECONV_CASES))
def test_deconv_bound_rejects_swapped_parity_offsets(cid):
    c = bc.BY_ID[cid]
    x, sd, _ = bc.deconv_tensors(cid)
    w, b = bc.deconv_folded(sd)
    ref, S = bc.deconv_reference(cid, False, False)
    assert _worst(bc.deconv_by_parity(x, w, b, c.k, swap=True), ref, bc.fp32_bound(c.K, S)) >= REJECT


@pytest.mark.parametrize("cid", [c.id for c in bc.FUSE_CASES if c.dt and len(c.scales) == 2])
def test_fuse_reference_rejects_the_other_order(cid):
    """(base + t2) + t1 rounds differently from (base + t1) + t2 often enough to show after the rounding to 16 bit"""
    c = bc.BY_ID[cid]
    base, terms = bc.fuse_tensors(cid)
    for act in (0, 1):
        a = bc.fuse_value(base, terms, c.scales, act, c.dt)
        b = bc.fuse_value(base, terms, c.scales, act, c.dt, order=(1, 0))
        assert a.dtype == bc.TDT[c.dt] and (a != b).any()


# ---- coverage ----
def _stem_dispatch(cin, cout, dt):
    """i2r_stem_conv (csrc/i2r_misc.hip): `if (cout == 64)` -> mf[cin == 3][out_dt], else fns[cin == 3][out_dt]"""
    return "%s<%d, %d>" % ("stem_mfma_k" if cout == 64 else "stem_conv_k", 3 if cin == 3 else 1, dt)


def _head_dispatch(cin, cout, hw, npix):
    """i2r_head: `cin % 16 == 0 && cin <= 128 && npix + 256 < 2^31` -> head_mfma_k<cout <= 16 ? 1 : 2>, whose lanes store 16 bytes when
    `(hw & 3) == 0` (then npix is a multiple of 4 too and `pd + 3 < total` holds for every lane with a pixel); else head_k<JP>,
    JP = cout <= 16 ? 16 : cout <= 20 ? 20 : 32"""
    if cin % 16 == 0 and cin <= 128 and npix + 256 < (1 << 31):
        return "head_mfma_k<%d>/%s" % (1 if cout <= 16 else 2, "scalar" if hw & 3 else "vector")
    return "head_k<%d>" % (16 if cout <= 16 else 20 if cout <= 20 else 32)


def test_every_instantiation_has_a_case():
    assert all(bc.stem_kernel(c.cin, c.cout, dt) == _stem_dispatch(c.cin, c.cout, dt) for c in bc.STEM_CASES for dt in (0, 1, 2))
    assert all(bc.head_kernel(c.cin, c.cout, c.h * c.w, c.n * c.h * c.w) == _head_dispatch(c.cin, c.cout, c.h * c.w, c.n * c.h * c.w) for c in bc.HEAD_CASES)
    stem = {bc.stem_kernel(c.cin, c.cout, dt) for c in bc.STEM_CASES for dt in (0, 1, 2)}
    assert stem == {"%s<%d, %d>" % (k, cin, dt) for k in ("stem_conv_k", "stem_mfma_k") for cin in (1, 3) for dt in (0, 1, 2)} and len(stem) == 12
    assert {c.cout // 16 for c in bc.STEM_CASES if c.cout != 64} == {1, 2, 8}           # channel groups of the VALU kernel
    for cin in (1, 3):
        for cout in bc.STEM_COUTS:
            assert {(c.n, c.h, c.w, c.n_src, c.n_valid) for c in bc.STEM_CASES if (c.cin, c.cout) == (cin, cout)} == set(bc.STEM_INPUTS)
    head = {bc.head_kernel(c.cin, c.cout, c.h * c.w, c.n * c.h * c.w) for c in bc.HEAD_CASES}
    assert head == {"head_k<16>", "head_k<20>", "head_k<32>", "head_mfma_k<1>/vector", "head_mfma_k<1>/scalar", "head_mfma_k<2>/vector",
                    "head_mfma_k<2>/scalar"}
    valu = [c for c in bc.HEAD_CASES if bc.head_kernel(c.cin, c.cout, c.h * c.w, c.n * c.h * c.w).startswith("head_k")]
    assert any((c.cin // 4) % 4 for c in valu) and any(c.cout == 1 for c in valu) and any(c.in_cs > c.cin for c in valu)
    assert all(bc.head_lds_bytes(c.cin, c.cout) <= 64 * 1024 for c in valu)
    mfma = [c for c in bc.HEAD_CASES if c not in valu]
    assert any(c.n * c.h * c.w < 16 for c in mfma) and any(c.cin == 16 for c in mfma) and any(c.in_cs > c.cin for c in mfma)
    assert {bc.fuse_kernel(c.dt) for c in bc.FUSE_CASES} == {"fuse_up_add_k<0>", "fuse_up_add_k<1>", "fuse_up_add_k<2>"}
    assert {s for c in bc.FUSE_CASES for s in c.scales} == {2, 4, 8} and {c.cs for c in bc.FUSE_CASES} == {4, 48}
    assert {c.k for c in bc.DECONV_CASES} == set(bc.Packer.DECONV_TAPS) == set(bc.DECONV_CFG)
    assert {c.rate for c in bc.CAT_CASES} == {0, 2, 3} and {c.vec for c in bc.CAT_CASES} == {40, 300} and {c.c0 for c in bc.CAT_CASES} == {0, 78}
    assert all(c.c_end < c.out_cs and c.n == 2 * c.n_src and c.n_valid < c.n_src for c in bc.CAT_CASES)
    assert any(c.n_valid < c.n_src for c in bc.PE_RES_CASES) and {c.out_cs for c in bc.PE_RES_CASES} == {64, 80}
    assert any(c.c < c.in_cs != c.out_cs for c in bc.POOL_CASES)


# ---- the inputs are instructive ----
def _uninstructive(ref, bound):
    return (bound < 1e-6 * ref.abs().max()).float().mean().item()


@pytest.mark.parametrize("cid", bc.ids(bc.STEM_CASES + bc.PE_RES_CASES + bc.HEAD_CASES + bc.CAT_CASES + bc.DECONV_CASES))
def test_inputs_are_instructive(cid):
    """at most 5 % of a case's elements may have a bound below 1e-6 of the largest value of its map"""
    c = bc.BY_ID[cid]
    if c in bc.STEM_CASES:
        ref, S = bc.stem_reference(cid)
        pairs = [(ref, bc.fp32_bound(c.K, S))]
    elif c in bc.PE_RES_CASES:
        pairs = [bc.pe_res_reference(cid)]
    elif c in bc.HEAD_CASES:
        ref, S = bc.head_reference(cid)
        pairs = [(ref, bc.fp32_bound(c.K, S))]
    elif c in bc.CAT_CASES:
        ref, S = bc.cat_reference(cid)
        pairs = [(ref, bc.fp32_bound(c.K, S))]
    else:
        pairs = []
        for relu in (False, True):
            for post in (False, True):
                ref, S = bc.deconv_reference(cid, relu, post)
                pairs.append((ref, bc.fp32_bound(c.K, S)))
    for ref, bound in pairs:
        assert ref.abs().max().item() > 0
        share = _uninstructive(ref, bound)
        assert share <= 0.05, "%s: %.1f %% of the elements are bounded below 1e-6 max |ref|" % (cid, 100 * share)
