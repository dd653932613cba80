"""Descriptor-level cases for the implicit-GEMM convolution family (csrc/i2r_conv.hip, i2r_conv_lp.inc) and their float64 reference.

The kernels are a family conv_igemm_f32<MT, NT, CAP, PF> / conv_igemm_lp<MT, NT, CAP, PF> (bf16, f16): MT 1..4 x NT 3, 4, 5 x
(CAP, PF) in {(4, 0), (4, 1), (12 | 8, 1), (4, 2)} = 144 instantiations, picked at run time by prepare() / resolve() (csrc/i2r_conv_plan.h) from the descriptor.
This module holds, for every instantiation, at least one descriptor that resolves to it and stresses what differs between the
instantiations (partial M fragments, partial tiles, several channel chunks with odd and even counts, padded output channels, several
channel blocks), plus grouped launches that force the members onto a common staging variant.  tests/test_conv_dispatch.py checks on the
CPU that every case resolves to the instantiation it names and that everything the engine launches is covered; tests/test_kernels_gpu.py
runs every case against reference() on the GPU.

Nothing here goes through engine.Program or calls into csrc/ for the expected values: reference() is the formula of the header comment
of i2r_conv_desc (include/i2r_hip.h) in float64 with plain torch ops."""
import ctypes as C
import math
import types
import zlib

import torch

from i2r_amd import cabi, engine

TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DT_NAME = {0: "fp32", 1: "bf16", 2: "f16"}
SENTINEL = 7.0   # exactly representable in fp32, bf16 and f16
GUARD = 2        # guard rows (of out_w pixels) in front of and behind every output tensor

MTS, NTS = (1, 2, 3, 4), (3, 4, 5)


def variants(dtype):
    """(CAP, PF) pairs the kernels are built for: i2r_pick_conv_f32 (csrc/i2r_conv.hip) / pick_lp (csrc/i2r_conv_lp.inc)"""
    wide = 12 if dtype == 0 else 8
    return ((4, 0), (4, 1), (wide, 1), (4, 2))


def kernel_name(dtype, mt, nt, cap, pf):
    """the instantiation's name as i2r_conv_kernel_name prints it"""
    if dtype == 0:
        return "conv_igemm_f32<%d, %d, %d, %d>" % (mt, nt, cap, pf)
    return "conv_igemm_lp<%d, %d, %d, %d>/%s" % (mt, nt, cap, pf, DT_NAME[dtype])


def all_names():
    """the full family, generated from the template parameter lists"""
    return {kernel_name(dt, mt, nt, cap, pf) for dt in (0, 1, 2) for mt in MTS for nt in NTS for cap, pf in variants(dt)}


# ------------------------------------------------------------------------------------------------------------------------------
# descriptor
# ------------------------------------------------------------------------------------------------------------------------------
def make_desc(*, n_img, in_h, in_w, in_cs, cin, conv_h, conv_w, out_h, out_w, out_cs, cout, cout_pad, stride, iy0, ix0, taps,
              tile_h=0, tile_w=0, mt=0, wn=0, ck=0, dtype=0, in_f16=0, out_f16=0, relu=0, out_step=1, out_off_y=0, out_off_x=0, rep=1,
              algo=0, in_=0x10000, in2=None, w=0x20000, bias=0x30000, res1=None, res2=None, res_post=None, out=0x40000):
    """A raw cabi.ConvDesc from explicit arguments.  The pointer arguments are integers (device addresses); their defaults are distinct
    non-null placeholders, which is all the host-side resolver (i2r_conv_kernel_name) looks at, so this works without a GPU."""
    d = cabi.ConvDesc()
    d.in_, d.in2, d.w, d.bias, d.res1, d.res2, d.res_post, d.out = in_, in2, w, bias, res1, res2, res_post, out
    d.n_img, d.in_h, d.in_w, d.in_cs, d.cin = n_img, in_h, in_w, in_cs, cin
    d.conv_h, d.conv_w, d.out_h, d.out_w, d.out_cs = conv_h, conv_w, out_h, out_w, out_cs
    d.cout, d.cout_pad, d.stride, d.iy0, d.ix0 = cout, cout_pad, stride, iy0, ix0
    d.ntaps = len(taps)
    for i, (dy, dx) in enumerate(taps[:cabi.MAX_TAPS]):
        d.dy[i], d.dx[i] = dy, dx
    d.out_step, d.out_off_y, d.out_off_x, d.rep, d.relu = out_step, out_off_y, out_off_x, rep, relu
    d.tile_h, d.tile_w, d.ck, d.wn, d.mt, d.dtype = tile_h, tile_w, ck, wn, mt, dtype
    d.in_f16, d.out_f16, d.algo = in_f16, out_f16, algo
    return d


def pack_weights(c, w_taps):
    """[ntaps, cin, cout] float64 -> the layout the kernels read, by the engine's own packers"""
    if c.dtype == 0:
        return engine.pack_k4(w_taps, c.cin, c.cout_pad)
    return engine.pack_k8(w_taps, c.cin, c.cout_pad, TDT[c.dtype])


def resolve(descs):
    """-> (rc, resolved name or None, error message) of i2r_conv_kernel_name for a list of descriptors; launches nothing"""
    L = cabi.lib()
    arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
    buf = C.create_string_buffer(96)
    rc = L.i2r_conv_kernel_name(arr, len(descs), buf, 96)
    if rc != 0:
        return rc, None, (L.i2r_last_error() or b"").decode()
    return 0, buf.value.decode(), ""


class Case(types.SimpleNamespace):
    """one convolution: the explicit descriptor arguments + which optional operands exist + the instantiation it is meant to resolve to"""

    def desc_args(self):
        return dict(n_img=self.n, in_h=self.in_h, in_w=self.in_w, in_cs=self.in_cs, cin=self.cin, conv_h=self.conv_h, conv_w=self.conv_w,
                    out_h=self.out_h, out_w=self.out_w, out_cs=self.out_cs, cout=self.cout, cout_pad=self.cout_pad, stride=self.stride,
                    iy0=self.iy0, ix0=self.ix0, taps=self.taps, tile_h=self.tile_h, tile_w=self.tile_w, mt=self.mt, wn=self.wn, ck=self.ck,
                    dtype=self.dtype, in_f16=self.in16, out_f16=self.out16, relu=self.relu, out_step=self.out_step,
                    out_off_y=self.out_off[0], out_off_x=self.out_off[1], rep=self.rep)

    def desc(self, **ptrs):
        """placeholder pointers for the operands the case has, unless `ptrs` gives real ones"""
        a = self.desc_args()
        if self.in2:
            a["in2"] = 0x50000
        if self.nres >= 1:
            a["res1"] = a.get("out", 0x40000) if self.inplace else 0x60000
        if self.nres >= 2:
            a["res2"] = 0x70000
        if self.res_post:
            a["res_post"] = 0x80000
        a.update(ptrs)
        return make_desc(**a)

    @property
    def id(self):
        return "%s-%s" % (self.name.replace("conv_igemm_", "").replace(" ", ""), self.tag)

    def describe(self):
        return ("%d x [%d x %d x %d/%d] -> conv %d x %d, %d taps stride %d -> [%d x %d x %d/%d/%d]; tile %d x %d mt %d wn %d ck %d; relu %d, "
                "res %d%s%s%s, step %d off %r rep %d, in16 %d out16 %d" % (
                    self.n, self.in_h, self.in_w, self.cin, self.in_cs, self.conv_h, self.conv_w, len(self.taps), self.stride, self.out_h,
                    self.out_w, self.cout, self.cout_pad, self.out_cs, self.tile_h, self.tile_w, self.mt, self.wn, self.ck, self.relu, self.nres,
                    " (in place)" if self.inplace else "", " + in2" if self.in2 else "", " + res_post" if self.res_post else "",
                    self.out_step, self.out_off, self.rep, self.in16, self.out16))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
def _rng(tag):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


def _sym(shape, g, scale=1.0):
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) * scale


def make_tensors(c):
    """CPU operands of a case, each in the type it is STORED in: x (and x2) [n, in_h, in_w, in_cs] (16 bit when in16), the residuals
    [n, out_h, out_w, out_cs] (16 bit when out16), w_taps [ntaps, cin, cout] float64 (scaled like the conv tests of test_kernels_gpu.py),
    bias [cout_pad] fp32.  Channels cin.. of x and the bias entries cout.. are random too: the kernels must not let them through."""
    g = _rng(c.tag + c.name)
    t = {}
    sin, sout = (TDT[c.dtype] if c.in16 else torch.float32), (TDT[c.dtype] if c.out16 else torch.float32)
    t["x"] = _sym((c.n, c.in_h, c.in_w, c.in_cs), g).to(sin)
    if c.in2:
        t["x2"] = _sym((c.n, c.in_h, c.in_w, c.in_cs), g).to(sin)
    t["w_taps"] = _sym((len(c.taps), c.cin, c.cout), g, (6.0 / (c.cin * len(c.taps))) ** 0.5)
    t["bias"] = _sym((c.cout_pad,), g, 0.3).float()
    for i, key in enumerate(("res1", "res2")):
        if c.nres > i:
            t[key] = _sym((c.n, c.out_h, c.out_w, c.out_cs), g).to(sout)
    if c.res_post:
        t["res_post"] = _sym((c.n, c.out_h, c.out_w, c.out_cs), g).to(sout)
    return t


def owned_mask(c):
    """[out_h, out_w] bool: the destination pixels the descriptor writes"""
    own = torch.zeros(c.out_h, c.out_w, dtype=torch.bool)
    for ry in range(c.rep):
        for rx in range(c.rep):
            own[(torch.arange(c.conv_h) * c.out_step + c.out_off[0] + ry)[:, None], (torch.arange(c.conv_w) * c.out_step + c.out_off[1] + rx)[None, :]] = True
    return own


def reference(c, t):
    """-> (expected [n, out_h, out_w, cout] float64, owned [out_h, out_w] bool): the header formula of i2r_conv_desc in float64.
    For the 16-bit operand types the activations and weights are first rounded to the type (that is what the matrix pipe multiplies);
    residuals enter as stored."""
    q = (lambda a: a.float().to(TDT[c.dtype]).double()) if c.dtype else (lambda a: a.float().double())
    x = t["x"][..., :c.cin].double()
    if c.in2:
        x = x + t["x2"][..., :c.cin].double()
    x = q(x)
    w = q(t["w_taps"])
    P = 4
    xp = torch.zeros(c.n, c.in_h + 2 * P, c.in_w + 2 * P, c.cin, dtype=torch.float64)
    xp[:, P:P + c.in_h, P:P + c.in_w] = x
    s = c.stride
    acc = torch.zeros(c.n, c.conv_h, c.conv_w, c.cout, dtype=torch.float64)
    for ti, (dy, dx) in enumerate(c.taps):
        y0, x0 = c.iy0 + dy + P, c.ix0 + dx + P
        y1, x1 = y0 + (c.conv_h - 1) * s, x0 + (c.conv_w - 1) * s
        assert y0 >= 0 and x0 >= 0 and y1 < xp.shape[1] and x1 < xp.shape[2], "reference padding too small for the case"
        acc += xp[:, y0:y1 + 1:s, x0:x1 + 1:s] @ w[ti]
    v = acc + t["bias"][:c.cout].double()
    exp = torch.zeros(c.n, c.out_h, c.out_w, c.cout, dtype=torch.float64)
    own = torch.zeros(c.out_h, c.out_w, dtype=torch.bool)
    for ry in range(c.rep):
        for rx in range(c.rep):
            ys = (torch.arange(c.conv_h) * c.out_step + c.out_off[0] + ry)[:, None]
            xs = (torch.arange(c.conv_w) * c.out_step + c.out_off[1] + rx)[None, :]
            r = v.clone()
            for key in ("res1", "res2"):
                if key in t:
                    r = r + t[key][:, ys, xs][..., :c.cout].double()
            if c.relu == 1:
                r = r.clamp_min(0.0)
            elif c.relu == 2:
                r = 0.5 * r * (1.0 + torch.erf(r / math.sqrt(2.0)))
            if c.res_post:
                r = r + t["res_post"][:, ys, xs][..., :c.cout].double()
            assert not own[ys, xs].any()
            exp[:, ys, xs] = r
            own[ys, xs] = True
    return exp, own


def initial_out(c, t):
    """the guarded output buffer before the launch, [GUARD + n * out_h + GUARD, out_w, out_cs] in the output's storage type: the
    sentinel everywhere; a case that accumulates in place (res1 == out) carries its residual in channels < cout of the pixels it owns"""
    sout = TDT[c.dtype] if c.out16 else torch.float32
    buf = torch.full((2 * GUARD + c.n * c.out_h, c.out_w, c.out_cs), SENTINEL, dtype=sout)
    if c.inplace:
        body = buf[GUARD:GUARD + c.n * c.out_h].view(c.n, c.out_h, c.out_w, c.out_cs)
        own = owned_mask(c)
        body[:, own, :c.cout] = t["res1"][:, own, :c.cout]
    return buf


def check_output(c, t, buf):
    """buf: the guarded buffer after the launch (CPU).  Asserts values, sentinels and padding; -> (max error, bar) for reports."""
    g = buf.double()
    assert (g[:GUARD] == SENTINEL).all() and (g[-GUARD:] == SENTINEL).all(), "%s: guard rows written" % c.id
    body = g[GUARD:-GUARD].view(c.n, c.out_h, c.out_w, c.out_cs)
    exp, own = reference(c, t)
    assert (body[:, ~own] == SENTINEL).all(), "%s: destination pixels the descriptor does not own were written" % c.id
    got, ref = body[:, own][..., :c.cout], exp[:, own]
    err = (got - ref).abs()
    if c.dtype == 0:
        bar = 2e-5 * max(1.0, ref.abs().max().item())   # fp32 against float64 (test_conv_winograd_matches_torch_and_direct)
        ok = err.max().item() < bar
    elif not c.out16:
        bar = 5e-4                                      # 16-bit operands, fp32 accumulate and store (test_conv_low_precision)
        ok = err.max().item() < bar
    else:
        ulp = 2.0 ** -8 if c.dtype == 1 else 2.0 ** -11  # result rounded once to the type (test_conv_16bit_activation_storage)
        bar = (ulp * ref.abs() + 5e-4)
        ok = bool((err <= bar).all())
        bar = bar.max().item()
    print("%s: max |got - ref| %.3e (bar %.3e, max |ref| %.3f)" % (c.id, err.max().item(), bar, ref.abs().max().item()))
    assert ok, "%s: max |got - ref| %.3e exceeds %.3e (%s)" % (c.id, err.max().item(), bar, c.describe())
    if c.out_cs >= c.cout_pad:
        assert (body[:, own][..., c.cout:c.cout_pad] == 0.0).all(), "%s: padding channels cout .. cout_pad - 1 must be exactly zero" % c.id
        assert (body[:, own][..., c.cout_pad:] == SENTINEL).all(), "%s: channels past cout_pad written" % c.id
    return err.max().item(), bar


def launch_args(c, t, dev):
    """device operands of a case -> (descriptor, guarded output tensor, keep-alive list)"""
    esz = 2 if c.out16 else 4
    out = initial_out(c, t).to(dev)
    optr = out.data_ptr() + GUARD * c.out_w * c.out_cs * esz
    keep = {k: v.to(dev) for k, v in t.items() if k not in ("w_taps", "res1" if c.inplace else "")}
    keep["w"] = pack_weights(c, t["w_taps"]).to(dev)
    ptrs = dict(in_=keep["x"].data_ptr(), w=keep["w"].data_ptr(), bias=keep["bias"].data_ptr(), out=optr)
    if c.in2:
        ptrs["in2"] = keep["x2"].data_ptr()
    if c.nres >= 1:
        ptrs["res1"] = optr if c.inplace else keep["res1"].data_ptr()
    if c.nres >= 2:
        ptrs["res2"] = keep["res2"].data_ptr()
    if c.res_post:
        ptrs["res_post"] = keep["res_post"].data_ptr()
    return c.desc(**ptrs), out, keep


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
# cout_pad for (NT, wn, channel blocks per workgroup column): NT is the first of 3, 4, 5 that divides cout_pad / 16 (prepare()), wn
# must divide cout_pad / 16 / NT, n_cblk = cout_pad / 16 / (NT * wn).  NT = 5 cannot have wn = 4 (20 fragments resolve to NT = 4).
COUT_PAD = {(3, 1, 1): 48, (3, 1, 2): 96, (3, 2, 1): 96, (3, 2, 2): 192, (3, 4, 1): 192,
            (4, 1, 1): 64, (4, 1, 2): 128, (4, 2, 1): 128, (4, 2, 2): 256, (4, 4, 1): 256,
            (5, 1, 1): 80, (5, 1, 2): 160, (5, 2, 1): 160}

FEATURES = ("relu", "in2", "res1", "res2", "inplace", "gelu", "post", "up2", "up4", "deconv", "plain")


def patch_of(th, tw, k, s):
    return ((th - 1) * s + k) * ((tw - 1) * s + k)


def pick_tile(mt, wm, k, s, lo, hi, full):
    """the squarest tile of a wm x mt workgroup (capacity wm * mt * 16 pixels) whose input patch has lo..hi pixels; full: the tile fills
    every M fragment, else its pixel count is no multiple of 16 and ends inside the last fragment (full None: anything that needs mt
    fragments per wave -- whole waves may then be idle, as in the engine's own choices for small maps).  None when there is none."""
    cap = wm * mt * 16
    best = None
    for th in range(2, 33):
        for tw in range(2, 49):
            px = th * tw
            if full is None:
                if not (mt - 1) * wm * 16 < px <= cap:
                    continue
            elif (px != cap) if full else not (cap - 16 < px < cap and px % 16):
                continue
            if not lo <= patch_of(th, tw, k, s) <= hi:
                continue
            key = (abs(th - tw), th) if full is not None else (-px, abs(th - tw), th)
            if best is None or key < best[0]:
                best = (key, th, tw)
    return best and best[1:]


def chunking(dtype, cin, plane, pf, cap, ck):
    """(channels per chunk, number of chunks) as prepare() derives them; `cap` is the kernel's prefetch capacity (a grouped launch may
    impose a wider one than the member would pick alone)"""
    g_ch = 4 if dtype == 0 else 8
    cin_g = cin // 4 if dtype == 0 else (cin // 8 + 3) // 4 * 4
    if pf > 0:
        lim = cap if pf == 1 else 4
        ckg = next((cand for cand in (12, 8, 4) if cand <= lim and cin_g % cand == 0 and 2 * cand * plane * 16 <= 40 * 1024), 4)
        return ckg * g_ch, cin_g // ckg
    if dtype != 0:
        fit = max(4, (24 * 1024 // (plane * 16)) // 4 * 4)
        nchunk = -(-cin_g // fit)
        ckg = -(-(-(-cin_g // nchunk)) // 4) * 4
        return ckg * 8, -(-cin_g // ckg)
    if ck == 0:
        fit = (20 * 1024 // (plane * 16)) * 4
        fit = 16 if fit < 16 else fit // 16 * 16
        ck = -(-(-(-cin // -(-cin // fit))) // 16) * 16
    return ck, -(-cin // ck)


def conv_case(dtype, name, tag, *, mt, wn, cout_pad, th, tw, k, s, cin, feature="plain", ck=0, in16=0, out16=0, parity=(0, 0), wide_cs=0,
              even_in=False, n=2):
    """One case from its blocking and filter: the conv map is 1.5 tiles high and two tiles minus one pixel wide (never a multiple of the
    tile), n images; cout = cout_pad - 6 (the last 16-byte channel piece is half padding); stride-2 inputs are odd unless even_in.
    wide_cs: 0 -> out_cs = cout_pad and in_cs = cin; 1 -> both 16 wider (channels past cout_pad / cin exist and must be left alone /
    unread); 2 -> out_cs = cout rounded up to 4 (< cout_pad: the padding pieces do not exist in the destination)."""
    c = Case(name=name, tag=tag, dtype=dtype, feature=feature, mt=mt, wn=wn, tile_h=th, tile_w=tw, ck=ck, in16=in16, out16=out16, n=n,
             cin=cin, cout_pad=cout_pad, cout=cout_pad - 6, stride=s, in2=False, nres=0, inplace=False, res_post=False, relu=0,
             out_step=1, out_off=(0, 0), rep=1)
    c.conv_h, c.conv_w = th + max(1, th // 2), 2 * tw - 1
    if feature == "deconv":  # ConvTranspose2d(k4, s2, p1) output parity (py, px): 2x2 taps over the input shifted by the parity, results interleaved
        assert k == 2 and s == 1
        c.taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
        c.iy0, c.ix0 = parity[0] - 1, parity[1] - 1
        c.in_h, c.in_w = c.conv_h, c.conv_w
        c.out_step, c.out_off, c.relu = 2, tuple(parity), 1
    else:
        c.taps = [(dy, dx) for dy in range(k) for dx in range(k)]
        c.iy0 = c.ix0 = -(k // 2)
        if s == 1:
            c.in_h, c.in_w = c.conv_h, c.conv_w
        else:
            c.in_h, c.in_w = 2 * c.conv_h - (0 if even_in else 1), 2 * c.conv_w - (0 if even_in else 1)
    if feature == "relu":
        c.relu = 1
    elif feature == "in2":
        c.in2, c.relu = True, 1
    elif feature == "res1":
        c.nres, c.relu = 1, 1
    elif feature == "res2":
        c.nres = 2
    elif feature == "inplace":
        c.nres, c.inplace, c.relu = 1, True, 1
    elif feature == "gelu":
        c.relu = 2
    elif feature == "post":
        c.relu, c.res_post = 1, True
    elif feature == "res2post":
        c.nres, c.relu, c.res_post = 2, 1, True
    elif feature == "up2":  # nearest-upsample scatter accumulating onto a residual (the HRNet fuse sums)
        c.rep = c.out_step = 2
        c.nres, c.relu = 1, 1
    elif feature == "up4":
        c.rep = c.out_step = 4
        c.nres, c.inplace = 1, True
    c.out_h, c.out_w = c.conv_h * c.out_step, c.conv_w * c.out_step
    c.in_cs = cin + (16 if wide_cs == 1 else 0)
    c.out_cs = cout_pad + 16 if wide_cs == 1 else (c.cout + 3) // 4 * 4 if wide_cs == 2 else cout_pad
    c.n_cblk = cout_pad // 16 // (wn * next(x for x in NTS if cout_pad // 16 % x == 0))
    c.patch = patch_of(th, tw, len({dy for dy, _ in c.taps}), s)
    c.full = th * tw == (4 // wn) * mt * 16
    return c


_n_deconv = {0: 0, 1: 0, 2: 0}  # deconv cases built so far per dtype: their output parity walks through {0, 1}^2


def lp_features():
    return tuple("res2post" if f == "in2" else f for f in FEATURES)


def auto_case(dtype, mt, nt, cap, pf, i, feature=None, wn=None, tag_extra=""):
    """A case whose descriptor, launched alone, resolves to <mt, nt, cap, pf> of `dtype`.  i: running index that rotates everything the
    instantiation leaves open -- the feature (unless given), full / partial last fragment, odd / even chunk count, filter and stride,
    waves along cout (unless wn is given), channel blocks, channel strides, storage types.  None when no tile exists (only with wn given)."""
    wide = 12 if dtype == 0 else 8
    nti, vi = NTS.index(nt), variants(dtype).index((cap, pf))
    if feature is None:
        feats = FEATURES if dtype == 0 else lp_features()
        feature = feats[i % len(feats)]
        if feature == "deconv" and pf == 2:  # (the PF = 2 cases are stride-2 convs)
            feature = feats[(i + 1) % len(feats)]
    full = (nti + vi + mt) % 2 == 0
    even = ((nti + vi) // 2 + mt) % 2 == 0  # wanted parity of the chunk count
    big = pf == 0 and mt >= 2 and (nti + mt) % 2 == 0 and feature != "deconv"  # PF 0 through a patch above 512 pixels; else through ck
    # patch range of the variant: wide prefetch needs 2 * ckg * plane * 16 <= 40 KB of LDS (plane <= 160 slots for 8 groups)
    lo, hi = {(4, 0): (513, 1280) if big else (1, 256), (4, 1): (1, 256), (wide, 1): (1, 160), (4, 2): (257, 512)}[(cap, pf)]
    if feature == "deconv":
        filters = [(2, 1)]
    elif pf == 2:
        filters = [(3, 2), (1, 2), (3, 1)]  # stride 2 wherever a tile exists, as where the towers use these kernels
    elif big:
        filters = [(3, 2)]
    else:
        filters = [[(3, 1), (1, 1), (3, 2), (1, 2)], [(3, 2), (3, 1), (1, 2), (1, 1)], [(1, 1), (3, 1), (1, 2), (3, 2)]][i % 3]
        if (cap, pf) == (4, 1) and even:  # an even chunk count under CAP 4 needs a plane above 160 slots: stride-2 patches first
            filters, lo = [(3, 2), (1, 2), (3, 1), (1, 1)], 161
    wms = [4 // wn] if wn else [w for w in ([4, 2, 1][(i // 4) % 3:] + [4, 2, 1][:(i // 4) % 3]) if any((nt, 4 // w, b) in COUT_PAD for b in (1, 2))]
    lo1 = 1 if lo == 161 else lo
    # (a PF 2 tile with a stride-2 filter under any wave split comes before a stride-1 one)
    tries = ((wm, k, s, pick_tile(mt, wm, k, s, lo_, hi, full_))
             for flt in ([filters[:2], filters[2:]] if pf == 2 else [filters])
             for lo_, full_ in ((lo, full), (lo, not full), (lo1, full), (lo1, not full), (lo1, None))
             for wm in wms for k, s in flt)
    pick = next(((wm, k, s) + tile for wm, k, s, tile in tries if tile), None)
    if not pick:
        assert wn, "no tile for %s" % kernel_name(dtype, mt, nt, cap, pf)
        return None
    wm, k, s, th, tw = pick
    wn = 4 // wm
    nb = 2 if ((nt, wn, 2) in COUT_PAD and (i % 2 == 0 or (nt, wn, 1) not in COUT_PAD)) else 1
    cout_pad = COUT_PAD[(nt, wn, nb)]
    plane = -(-patch_of(th, tw, k, s) // 16) * 16
    ck = 0
    if dtype == 0:
        if pf == 0:
            cin, ck = 80, (0 if big else 32)             # ck 32: chunks of 32, 32, 16 channels (short last chunk)
        elif pf == 2:
            cin = 64 if even else 48
        elif cap == 4:
            cin = (64 if even else 48) if plane > 160 else 80  # plane <= 160: 20 groups, chunks of 4 (5 chunks)
        else:
            cin = (192 if even else 144) if plane <= 96 else (128 if even else 160)  # chunks of 12 groups; of 8 where 12 do not fit
    else:
        if pf == 0:
            cin, ck = (144 if big else 272 if even else 208), (0 if big else 64)  # 208: 26 groups of 8 channels padded to 28 (short last chunk)
        elif pf == 2:
            cin = 128 if even else (96 if i % 2 else 80)  # 80: 10 groups padded to 12
        elif cap == 4:
            cin = (128 if even else 96) if plane > 160 else (80 if i % 2 else 96)
        else:
            cin = 256 if even else (176 if i % 2 else 192)  # 176: 22 groups padded to 24
    sc = (i // 4 + i) % 4 if dtype else 0
    c = conv_case(dtype, kernel_name(dtype, mt, nt, cap, pf), "%s%s%s" % (feature, "" if not dtype else "-i%do%d" % (sc & 1, sc >> 1), tag_extra),
                  mt=mt, wn=wn, cout_pad=cout_pad, th=th, tw=tw, k=k, s=s, cin=cin, feature=feature, ck=ck, in16=sc & 1,
                  out16=sc >> 1, parity=((_n_deconv[dtype] >> 1) & 1, _n_deconv[dtype] & 1), wide_cs=i % 3, even_in=(pf != 2 and i % 2 == 1))
    _n_deconv[dtype] += feature == "deconv"
    c.chunks = chunking(dtype, cin, plane, pf, cap, ck)[1]
    c.variant = (cap, pf)
    return c


def _family_cases():
    """one case per instantiation, features spread over the table (every feature meets MT >= 2 in every dtype: MT is the outer loop)"""
    cases = []
    for dtype in (0, 1, 2):
        i = 0
        for mt in MTS:
            for nt in NTS:
                for cap, pf in variants(dtype):
                    cases.append(auto_case(dtype, mt, nt, cap, pf, i))
                    i += 1
    return cases


# (MT, NT, CAP, PF, wn) of the single launches the shipped towers resolve to with a `wn` the family table above does not pair with that
# instantiation (tests/test_conv_dispatch.py::test_engine_only_launches_what_the_cases_cover names what is missing when the engine's
# cost model moves).  "lp" rows are built for bf16 and f16, CAP 8 standing for the wide variant.
ENGINE_SINGLES = {
    "fp32": [(1, 3, 12, 1, 2), (1, 3, 12, 1, 4), (1, 4, 12, 1, 1), (1, 5, 12, 1, 2), (1, 5, 4, 1, 2), (2, 3, 12, 1, 2), (2, 3, 12, 1, 4),
             (2, 4, 12, 1, 1), (2, 4, 4, 1, 1), (2, 5, 12, 1, 2), (2, 5, 4, 1, 2), (3, 3, 12, 1, 4), (3, 4, 12, 1, 1), (3, 4, 12, 1, 4),
             (3, 4, 4, 1, 1), (3, 5, 4, 1, 2)],
    "lp": [(1, 3, 4, 1, 4), (1, 4, 8, 1, 1), (2, 4, 4, 1, 1), (2, 4, 8, 1, 1), (3, 4, 4, 1, 1), (3, 4, 8, 1, 4), (3, 5, 4, 1, 2), (4, 4, 4, 2, 1)],
}


def _engine_single_cases():
    cases = []
    for key, rows in ENGINE_SINGLES.items():
        for dtype in ((0,) if key == "fp32" else (1, 2)):
            for j, (mt, nt, cap, pf, wn) in enumerate(rows):
                c = auto_case(dtype, mt, nt, cap, pf, 5 * j + 3, wn=wn, tag_extra="-wn%d" % wn)
                assert c is not None, (key, mt, nt, cap, pf, wn)
                cases.append(c)
    return cases


CASES = _family_cases() + _engine_single_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# grouped launches
# ------------------------------------------------------------------------------------------------------------------------------
class GroupCase(types.SimpleNamespace):
    """members (Cases, each with its own output) of one i2r_conv_grouped launch, the dispatch table mode (None | "lpt" | "reversed" |
    "interleaved") and the instantiation resolve() must settle on for all of them"""

    @property
    def id(self):
        return "%s-wn%s-%s" % (self.name.replace("conv_igemm_", "").replace(" ", ""), "".join(str(m.wn) for m in self.members), self.map or "nomap")

    def counts(self):
        """workgroups per member"""
        return [m.n * -(-m.conv_h // m.tile_h) * -(-m.conv_w // m.tile_w) * m.n_cblk for m in self.members]

    def block_map(self):
        counts = self.counts()
        if self.map is None:
            return None
        if self.map == "lpt":
            return engine.lpt_block_order(counts, [m.cin * len(m.taps) for m in self.members])
        plain = [(g << 24) | i for g, n in enumerate(counts) for i in range(n)]
        if self.map == "reversed":
            return plain[::-1]
        assert self.map == "interleaved"  # round-robin over the members, each walking its workgroups backwards
        out, left = [], list(counts)
        while any(left):
            for g in range(len(counts)):
                if left[g]:
                    left[g] -= 1
                    out.append((g << 24) | left[g])
        return out

    @property
    def signature(self):
        return (self.name, tuple(m.wn for m in self.members), len(self.members), self.map is not None)


def auto_group(dtype, mt, nt, cap, pf, wns, map_mode, i=0, carrier_last=False):
    """Members that ALONE resolve to different staging variants and together are forced onto <mt, nt, cap, pf> (resolve(): the most general
    variant any member needs): the first member that can (the last one with carrier_last) carries the target variant, the others are
    narrow single-prefetch members (CAP 4, PF 1) -- so a PF 2 target mixes PF 1 + PF 2, a wide-CAP target runs members with 4 channel
    groups per chunk under the wide kernel, a PF 0 target drags double-buffered members onto synchronous staging."""
    feats = FEATURES if dtype == 0 else lp_features()
    feature = lambda j: feats[(3 * i + 4 * j + 2) % len(feats)]
    members = [None] * len(wns)
    for j in (reversed(range(len(wns))) if carrier_last else range(len(wns))):
        f = feature(j)
        members[j] = auto_case(dtype, mt, nt, cap, pf, i + j, wn=wns[j], feature="relu" if (f == "deconv" and pf == 2) else f, tag_extra="-g%d" % j)
        if members[j] is not None:
            break
    assert any(m is not None for m in members), (dtype, mt, nt, cap, pf, wns)
    for j, wn in enumerate(wns):
        if members[j] is None:
            members[j] = auto_case(dtype, mt, nt, 4, 1, i + j, wn=wn, feature=feature(j), tag_extra="-g%d" % j)
            assert members[j] is not None, (dtype, mt, nt, cap, pf, wns, j)
    return GroupCase(name=kernel_name(dtype, mt, nt, cap, pf), variant=(cap, pf), members=members, map=map_mode)


# grouped launches of the shipped towers as (MT, NT, CAP, PF, wn per member, dispatch table?); "lp" rows for bf16 and f16 (CAP 8 = wide)
ENGINE_GROUPS = {
    "fp32": [(1, 3, 12, 1, (2, 1), True), (1, 3, 12, 1, (2, 2, 2, 2), False), (1, 3, 12, 1, (4, 1, 2, 1), True), (1, 3, 4, 2, (4, 2, 1), True),
             (1, 5, 12, 1, (1, 2), False), (2, 3, 12, 1, (2, 2, 2, 2), False), (2, 3, 12, 1, (4, 1, 2, 1), True), (2, 3, 4, 2, (2, 1), True),
             (2, 5, 4, 2, (1, 2), False), (3, 3, 12, 1, (2, 2, 2, 2), False), (3, 3, 12, 1, (4, 1, 2, 1), True), (3, 3, 4, 2, (2, 1), True),
             (3, 5, 4, 2, (1, 2), False)],
    "lp": [(1, 3, 4, 1, (2, 2, 2, 2), False), (1, 3, 4, 2, (4, 2, 1), True), (1, 3, 8, 1, (1, 2), False), (1, 3, 8, 1, (2, 1), True),
           (1, 3, 8, 1, (4, 1, 2, 1), True), (1, 3, 8, 1, (4, 2, 1), True), (1, 5, 8, 1, (1, 2), False), (2, 3, 4, 1, (2, 1), True),
           (2, 3, 4, 1, (2, 2, 2, 2), False), (2, 3, 4, 2, (1, 2), False), (2, 3, 4, 2, (2, 1), True), (2, 3, 8, 1, (4, 1, 2, 1), True),
           (2, 3, 8, 1, (4, 2, 1), True), (2, 5, 4, 2, (1, 2), False), (3, 3, 4, 1, (2, 1), True), (3, 3, 4, 1, (2, 2, 2, 2), False),
           (3, 3, 4, 2, (1, 2), False), (3, 3, 4, 2, (2, 1), True), (3, 3, 8, 1, (4, 1, 2, 1), True), (3, 3, 8, 1, (4, 2, 1), True),
           (3, 5, 4, 2, (1, 2), False)],
}

# the forced-common-variant paths of resolve() beyond what the towers launch: any member on PF 0 -> all on PF 0 (through ck and through a
# patch above 512 pixels), MT 2 and 3, NT 4 and 5, hand-made dispatch orders
FORCED_GROUPS = [
    (0, 2, 3, 4, 2, (2, 1), None), (0, 3, 4, 12, 1, (2, 1, 2), "lpt"), (0, 3, 5, 4, 0, (1, 2), "interleaved"), (0, 2, 4, 4, 0, (2, 1, 1), "reversed"),
    (1, 2, 3, 4, 0, (1, 2), "reversed"), (1, 3, 4, 8, 1, (1, 2, 4, 1), "interleaved"), (2, 2, 4, 8, 1, (1, 2, 1, 2), "lpt"),
    (2, 3, 3, 4, 0, (2, 4, 1), "lpt"), (2, 2, 5, 4, 2, (2, 1), "reversed"),
]
# ... and with the member that needs the common variant LAST (resolve() must look at every member, not at the first)
FORCED_GROUPS_CARRIER_LAST = [(0, 2, 3, 12, 1, (1, 2), "lpt"), (0, 3, 5, 4, 2, (1, 2, 2), None), (1, 3, 3, 8, 1, (2, 1, 2), None), (2, 2, 4, 4, 0, (1, 2), "interleaved")]


def _group_cases():
    groups = [auto_group(dt, mt, nt, cap, pf, wns, mode, i=7 * j + 1) for j, (dt, mt, nt, cap, pf, wns, mode) in enumerate(FORCED_GROUPS)]
    groups += [auto_group(dt, mt, nt, cap, pf, wns, mode, i=5 * j + 2, carrier_last=True)
               for j, (dt, mt, nt, cap, pf, wns, mode) in enumerate(FORCED_GROUPS_CARRIER_LAST)]
    for key, rows in ENGINE_GROUPS.items():
        for dtype in ((0,) if key == "fp32" else (1, 2)):
            for j, (mt, nt, cap, pf, wns, has_map) in enumerate(rows):
                groups.append(auto_group(dtype, mt, nt, cap, pf, wns, "lpt" if has_map else None, i=5 * j + dtype))
    return groups


GROUP_CASES = _group_cases()
