"""-m gpu: the boundary kernels of csrc/i2r_misc.hip through the raw C ABI, and Packer.deconv / one case per family through
engine.Program, against the float64 references and derived bounds of tests/_boundary_cases.py.  Every output starts as NaN between two
guard zones, with a sentinel in the channels the kernel does not own and NaN in the input channels it must not read."""
import ctypes as C

import pytest
import torch

import _boundary_cases as bc
from _gpu_util import NAN_WORD, act_nchw, run_poisoned, to_act, tracked_program
from i2r_amd import cabi, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64   # 32-bit words in front of and behind every output


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    return t.contiguous().to(DEV)


class Out:
    """An output of `shape` elements of storage type dt between two guard zones.  Everything is NaN (NAN_WORD) but the elements outside
    `owned` (a bool tensor that broadcasts to shape), which hold SENTINEL; init: contents to start from instead (in-place operands)."""

    def __init__(self, shape, dt, owned=None, init=None):
        n_el = 1
        for s in shape:
            n_el *= s
        words = n_el if dt == 0 else (n_el + 1) // 2
        self.raw = torch.full((GUARD + words + GUARD,), NAN_WORD, dtype=torch.int32, device=DEV)
        self.body = self.raw[GUARD:GUARD + words].view(bc.TDT[dt])[:n_el].view(shape)
        self.owned = torch.ones(shape, dtype=torch.bool) if owned is None else owned.expand(shape).clone()
        if init is not None:
            self.body.copy_(init.to(DEV))
        self.body[~self.owned.to(DEV)] = bc.SENTINEL
        self.before = self.raw.clone()
        self.words = words

    @property
    def ptr(self):
        return self.body.data_ptr()

    def untouched(self):
        return torch.equal(self.raw, self.before)

    def result(self):
        """the body on the CPU, after checking the guard zones, the sentinels and that every owned element was written with a finite value"""
        torch.cuda.synchronize()
        assert torch.equal(self.raw[:GUARD], self.before[:GUARD]), "the guard zone in front of the output was written"
        assert torch.equal(self.raw[GUARD + self.words:], self.before[GUARD + self.words:]), "the guard zone behind the output was written"
        b = self.body.cpu()
        assert (b[~self.owned] == bc.SENTINEL).all(), "elements the kernel does not own were written"
        assert torch.isfinite(b[self.owned].float()).all(), "owned elements unwritten or not finite"
        return b


def _owned_channels(shape, lo, hi):
    own = torch.zeros(shape, dtype=torch.bool)
    own[..., lo:hi] = True
    return own


def _nan_padded(x, cs):
    """[..., c] -> device [..., cs] with NaN in the channels c .. cs - 1"""
    buf = torch.full(tuple(x.shape[:-1]) + (cs,), float("nan"), dtype=x.dtype)
    buf[..., :x.shape[-1]] = x
    return _dev(buf)


def _within(name, got, ref, bound):
    ratio = ((got.double() - ref).abs() / bound).max().item()
    print("RATIO %s %.4f" % (name, ratio))
    assert got.shape == ref.shape
    assert ((got.double() - ref).abs() <= bound).all(), "%s: worst |got - ref| / bound = %.3f" % (name, ratio)


# ---- stem ----
def _stem_call(c, dt, x, w, b, out):
    return cabi.lib().i2r_stem_conv(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.ptr, c.n, c.cin, c.h, c.w, c.cout, c.out_cs, c.n_src, c.n_valid, dt, _stream())


@pytest.mark.parametrize("cid", bc.ids(bc.STEM_CASES))
def test_stem_conv(cid):
    """stem_conv_k (cout 16, 32, 128) and stem_mfma_k (cout 64): fp32 within fp32_bound(9 cin, S); bf16 / f16 outputs equal to the fp32
    output rounded once, bit for bit; channels cout .. out_cs - 1 untouched"""
    c = bc.BY_ID[cid]
    x, w, b = bc.stem_tensors(cid)
    xd, wd, bd = _dev(x), _dev(w.permute(2, 3, 1, 0).reshape(9, c.cin, c.cout)), _dev(b)
    shape = (c.n, (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1, c.out_cs)
    got = {}
    for dt in (0, 1, 2):
        out = Out(shape, dt, _owned_channels(shape, 0, c.cout))
        cabi.check(_stem_call(c, dt, xd, wd, bd, out), bc.stem_kernel(c.cin, c.cout, dt))
        got[dt] = out.result()[..., :c.cout]
    ref, S = bc.stem_reference(cid)
    _within("stem", got[0], ref, bc.fp32_bound(c.K, S))
    assert (got[0] >= 0).all()
    for dt in (1, 2):
        assert torch.equal(got[dt], got[0].to(bc.TDT[dt])), bc.stem_kernel(c.cin, c.cout, dt)


# ---- pe_res_stem ----
def _pe_res_operands(cid):
    m, w_pre, w7, b = bc.pe_res_tensors(cid)
    return _dev(m), _dev(w_pre.view(3, 9).t()), _dev(w7.permute(2, 3, 1, 0).reshape(147, 64)), _dev(b)


@pytest.mark.parametrize("cid", bc.ids(bc.PE_RES_CASES))
def test_pe_res_stem(cid):
    c = bc.BY_ID[cid]
    md, wp, w7, bd = _pe_res_operands(cid)
    shape = (c.n, (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1, c.out_cs)
    out = Out(shape, 0, _owned_channels(shape, 0, 64))
    cabi.check(cabi.lib().i2r_pe_res_stem(md.data_ptr(), wp.data_ptr(), w7.data_ptr(), bd.data_ptr(), out.ptr, c.n, c.h, c.w, 64, c.out_cs, c.n_src,
                                          c.n_valid, _stream()), "i2r_pe_res_stem")
    ref, bound = bc.pe_res_reference(cid)
    _within("pe_res", out.result()[..., :64], ref, bound)


# ---- max-pool ----
@pytest.mark.parametrize("cid", bc.ids(bc.POOL_CASES))
def test_maxpool(cid):
    """bit-exact; the input's channels c .. in_cs - 1 hold NaN, the output's c .. out_cs - 1 stay as they were"""
    c = bc.BY_ID[cid]
    xd = _nan_padded(bc.pool_tensors(cid), c.in_cs)
    shape = (c.n, (c.h - 1) // 2 + 1, (c.w - 1) // 2 + 1, c.out_cs)
    out = Out(shape, 0, _owned_channels(shape, 0, c.c))
    cabi.check(cabi.lib().i2r_maxpool3x3s2(xd.data_ptr(), out.ptr, c.n, c.h, c.w, c.c, c.in_cs, c.out_cs, _stream()), "i2r_maxpool3x3s2")
    assert torch.equal(out.result()[..., :c.c].double(), bc.pool_reference(cid))


# ---- head ----
def _head_run(c, x, w, b):
    xd, wd, bd = _nan_padded(x, c.in_cs), _dev(w), _dev(b)
    out = Out((c.n, c.cout, c.h, c.w), 0)
    cabi.check(cabi.lib().i2r_head(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, c.n, c.h, c.w, c.cin, c.in_cs, c.cout, _stream()), "i2r_head")
    return out.result()


@pytest.mark.parametrize("cid", bc.ids(bc.HEAD_CASES))
def test_head(cid):
    """head_mfma_k<1|2> (16-byte and scalar stores, fewer than 16 pixels, one 16-channel step) and head_k<16|20|32> (uneven shares of the
    quad lanes, one joint): within fp32_bound(cin, S), nothing written in front of or behind the planes"""
    c = bc.BY_ID[cid]
    ref, S = bc.head_reference(cid)
    _within(bc.head_kernel(c.cin, c.cout, c.h * c.w, c.n * c.h * c.w).split("<")[0], _head_run(c, *bc.head_tensors(cid)), ref, bc.fp32_bound(c.K, S))


def test_head_largest_weight_image_the_valu_kernel_accepts():
    """cin 512 x 32 joints: exactly 64 KB of LDS, the most i2r_head takes"""
    c = bc.Case(cin=512, cout=32, n=1, h=2, w=3, in_cs=512, K=512)
    assert bc.head_lds_bytes(c.cin, c.cout) == 64 * 1024 and bc.head_kernel(c.cin, c.cout, 6, 6) == "head_k<32>"
    x, w, b = bc.mags("head.big.x", (1, 2, 3, 512), 0.5), bc.weights("head.big.w", 32, (512,), 0.5, 0.2), bc.sym("head.big.b", (32,), 0.02)
    ref, S = bc.head_value(x, w, b)
    _within("head_k", _head_run(c, x, w, b), ref, bc.fp32_bound(c.K, S))


# ---- pe_cat_vec ----
def _cat_args(c, md, wd, bd, out, **over):
    a = cabi.PeCatVecArgs(md.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.ptr, c.n, c.h, c.w, c.th, c.tw, c.rate, c.vec, c.out_cs, c.c0, c.c_end, c.n_src,
                          c.n_valid)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("cid", bc.ids(bc.CAT_CASES))
def test_pe_cat_vec(cid):
    """channels [c0, c0 + vec) of every token row: the person's vector within fp32_bound(th tw, S); [c0 + vec, c_end): exact zeros;
    [0, c0) and [c_end, out_cs): untouched"""
    c = bc.BY_ID[cid]
    m, wfc, bfc = bc.cat_tensors(cid)
    md, wd, bd = _dev(m), _dev(wfc), _dev(bfc)
    shape = (c.n, c.th * c.tw, c.out_cs)
    out = Out(shape, 0, _owned_channels(shape, c.c0, c.c_end))
    cabi.check(cabi.lib().i2r_pe_cat_vec(C.byref(_cat_args(c, md, wd, bd, out)), _stream()), "i2r_pe_cat_vec")
    got = out.result()
    v, S = bc.cat_reference(cid)
    rep = lambda t: t.unsqueeze(1).expand(c.n, c.th * c.tw, c.vec)
    _within("pe_cat_vec", got[..., c.c0:c.c0 + c.vec], rep(v), rep(bc.fp32_bound(c.K, S)))
    assert (got[..., c.c0 + c.vec:c.c_end] == 0).all()
    assert torch.equal(got[:, :1, c.c0:c.c_end].expand(-1, c.th * c.tw, -1), got[..., c.c0:c.c_end])   # (one vector per person)


# ---- fuse_up_add ----
@pytest.mark.parametrize("cid", bc.ids(bc.FUSE_CASES))
def test_fuse_up_add(cid):
    """bit-exact for all three storage types (bc.fuse_value), with and without ReLU, out of place and in place (base aliases out)"""
    c = bc.BY_ID[cid]
    base, terms = bc.fuse_tensors(cid)
    td = [_dev(t) for t in terms]
    shape = (c.n, c.h, c.w, c.cs)
    for act in (0, 1):
        for inplace in (False, True):
            bd = Out(shape, c.dt, init=base)
            out = bd if inplace else Out(shape, c.dt)
            cabi.check(cabi.lib().i2r_fuse_up_add(bd.ptr, td[0].data_ptr(), c.scales[0], td[1].data_ptr() if len(td) > 1 else None,
                                                  c.scales[1] if len(td) > 1 else 1, out.ptr, c.n, c.h, c.w, c.cs, act, c.dt, _stream()), bc.fuse_kernel(c.dt))
            got = out.result()
            exp = bc.fuse_value(base, terms, c.scales, act, c.dt)
            assert got.dtype == exp.dtype and torch.equal(got, exp), "%s act %d in place %d: %d elements differ" % (cid, act, inplace, (got != exp).sum().item())
            if not inplace:
                assert bd.untouched()


# ---- deconv (Packer.deconv + Program.deconv) ----
@pytest.mark.parametrize("cid", bc.ids(bc.DECONV_CASES))
def test_deconv(cid):
    """ConvTranspose2d(k = 4, 3, 2) + BatchNorm as the packer's four parity convs, with and without ReLU and post-ReLU residual, against
    F.conv_transpose2d in float64: within fp32_bound(taps cin, S); poisoned buffers, pad channels zero, second run identical"""
    c = bc.BY_ID[cid]
    x, sd, post = bc.deconv_tensors(cid)
    P = tracked_program(torch.device(DEV))
    pcs = engine.Packer(sd, torch.device(DEV)).deconv("d", "b")
    xa, pa = to_act(P, x), to_act(P, post)
    keys = [(relu, wp) for relu in (False, True) for wp in (False, True)]
    outs = [P.deconv(xa, pcs, relu=relu, res_post=pa if wp else None) for relu, wp in keys]
    views = run_poisoned(P, [xa, pa], outs)
    for (relu, wp), o, v in zip(keys, outs, views):
        ref, S = bc.deconv_reference(cid, relu, wp)
        _within("deconv", act_nchw(o, v), ref, bc.fp32_bound(c.K, S))


# ---- one case per family through engine.Program ----
def test_engine_stem_and_pe_res():
    c = bc.BY_ID["stem-c3-o64-8x21x33-s4v3"]
    x, w, b = bc.stem_tensors(c.id)
    P = tracked_program(torch.device(DEV))
    st = dict(w=_dev(w.permute(2, 3, 1, 0).reshape(9, c.cin, c.cout)), bias=_dev(b), cin=c.cin, cout=c.cout)
    xd = _dev(x)
    out, args = P.stem(st, c.n, c.h, c.w, in_ptr=xd.data_ptr(), n_src=c.n_src)
    args.n_valid = c.n_valid
    r = bc.BY_ID["peres-17x18-mirror-cs80-s3v2"]
    md, wp, w7, bd = _pe_res_operands(r.id)
    out_r, args_r = P.pe_res_stem(dict(w_pre=wp, w7=w7, bias=bd, cout=64), r.n, r.h, r.w, n_src=r.n_src)
    args_r.in_, args_r.n_valid = md.data_ptr(), r.n_valid
    v, v_r = run_poisoned(P, [], [out, out_r])
    ref, S = bc.stem_reference(c.id)
    _within("stem", v[..., :c.cout].cpu(), ref, bc.fp32_bound(c.K, S))
    ref, bound = bc.pe_res_reference(r.id)
    _within("pe_res", v_r[..., :64].cpu(), ref, bound)


def test_engine_maxpool_head_and_fuse():
    P = tracked_program(torch.device(DEV))
    p = bc.BY_ID["pool-3x9x7-c12-16-32"]
    xp = bc.pool_tensors(p.id)
    pa = to_act(P, xp.permute(0, 3, 1, 2))
    pooled = P.maxpool(pa)
    h = bc.BY_ID["head-48-17-3x9x7"]
    x, w, b = bc.head_tensors(h.id)
    ha = to_act(P, x.permute(0, 3, 1, 2))
    assert ha.cs == h.cin
    heat = Out((h.n, h.cout, h.h, h.w), 0)
    P.head(ha, dict(w=_dev(w), bias=_dev(b), cin=h.cin, cout=h.cout), out_ptr=heat.ptr)
    f = bc.BY_ID["fuse-2+8-2x24x8x48-bf16"]
    base, terms = bc.fuse_tensors(f.id)
    fa = [to_act(P, t.float().permute(0, 3, 1, 2), f.dt) for t in [base] + terms]
    fused = P.fuse_up_add(fa[0], fa[1:], P.alloc(f.n, f.h, f.w, f.cs, f.dt), relu=True)
    v_pool, v_fuse = run_poisoned(P, [pa, ha] + fa, [pooled, fused])
    assert torch.equal(v_pool[..., :p.c].cpu().double(), bc.pool_reference(p.id))
    assert torch.equal(v_fuse.cpu(), bc.fuse_value(base, terms, f.scales, 1, f.dt))
    ref, S = bc.head_reference(h.id)
    _within("head_mfma_k", heat.result(), ref, bc.fp32_bound(h.K, S))


def test_engine_pe_cat_vec():
    c = bc.BY_ID["cat-50x44-r2-v40-c0"]
    m, wfc, bfc = bc.cat_tensors(c.id)
    P = tracked_program(torch.device(DEV))
    out = P.alloc(c.n, c.th, c.tw, c.vec)
    md = _dev(m)
    a = P.pe_cat_vec(dict(w=_dev(wfc), b=_dev(bfc), vec=c.vec), c.n, c.h, c.w, c.th, c.tw, out, 0, n_src=c.n_src)
    assert a.rate == c.rate
    a.in_, a.n_valid = md.data_ptr(), c.n_valid
    v, = run_poisoned(P, [], [out])
    ref, S = bc.cat_reference(c.id)
    rep = lambda t: t.view(c.n, 1, 1, c.vec).expand(c.n, c.th, c.tw, c.vec)
    _within("pe_cat_vec", v[..., :c.vec].cpu(), rep(ref), rep(bc.fp32_bound(c.K, S)))


# ---- argument errors: reported, nothing launched ----
def _refused(rc, out, what):
    torch.cuda.synchronize()
    assert rc == -1, "%s: rc %d" % (what, rc)
    msg = cabi.lib().i2r_last_error()
    assert msg and what.encode() in msg, msg
    assert out.untouched(), "%s wrote to its output although it refused the call" % what


def test_bad_arguments_are_refused_without_a_launch():
    L = cabi.lib()
    st = _stream()
    buf = torch.zeros(1 << 16, device=DEV)   # operands of every call below: large enough for what each call would read if it ran
    out = Out((1 << 14,), 0)
    p = buf.data_ptr()
    # stem: cout not a multiple of 16; a 16-bit row pitch that breaks the 16-byte stores; weights beyond 64 KB of LDS
    _refused(L.i2r_stem_conv(p, p, p, out.ptr, 1, 3, 8, 8, 24, 32, 1, 1, 0, st), out, "i2r_stem_conv")
    _refused(L.i2r_stem_conv(p, p, p, out.ptr, 1, 3, 8, 8, 16, 20, 1, 1, 1, st), out, "i2r_stem_conv")
    _refused(L.i2r_stem_conv(p, p, p, out.ptr, 1, 3, 2, 2, 592, 592, 1, 1, 0, st), out, "i2r_stem_conv")
    # head: more than 32 joints; a weight image beyond 64 KB of LDS for each of the three VALU kernels
    _refused(L.i2r_head(p, p, p, out.ptr, 1, 2, 2, 48, 48, 33, st), out, "i2r_head")
    for cin, cout in ((1028, 16), (820, 20), (516, 32)):
        assert bc.head_lds_bytes(cin, cout) > 64 * 1024 >= bc.head_lds_bytes(cin - 4, cout)
        _refused(L.i2r_head(p, p, p, out.ptr, 1, 2, 2, cin, cin, cout, st), out, "i2r_head")
    _refused(L.i2r_maxpool3x3s2(p, out.ptr, 1, 4, 4, 16, 16, 12, st), out, "i2r_maxpool3x3s2")
    _refused(L.i2r_fuse_up_add(p, p + 4096, 3, None, 1, out.ptr, 1, 6, 6, 16, 0, 0, st), out, "i2r_fuse_up_add")
    _refused(L.i2r_pe_res_stem(p, p, p, p, out.ptr, 1, 8, 8, 32, 32, 1, 1, st), out, "i2r_pe_res_stem")
    a = cabi.PeCatVecArgs(p, p, p, out.ptr, 1, 9, 7, 3, 1, 3, 8, 16, 0, 16, 1, 1)   # 9 x 7 pooled three times is 2 x 1
    _refused(L.i2r_pe_cat_vec(C.byref(a), st), out, "i2r_pe_cat_vec")
