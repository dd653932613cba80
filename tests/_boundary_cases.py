"""Cases and float64 references for the boundary kernels of csrc/i2r_misc.hip (stem conv, 'res' and 'cat_vec' position front ends,
max-pool, heat-map head, the closing pass of an HRNet fuse sum) and for the transposed-conv packing of pack.py (Packer.deconv).
Used on the CPU (tests/test_boundary_cases.py: the references restated a second way, wrong variants rejected, every instantiation
covered) and on the GPU (tests/test_boundary_gpu.py).

Nothing here calls into csrc/, engine.Program or oracle/ for an expected value: every reference is the definition of the operation in
float64 (F.conv2d, F.conv_transpose2d, F.max_pool2d, F.linear), and returns next to the value the per-element magnitude
S = sum |x_i w_i| + |bias| that the bound needs.

THE BOUND (fp32_bound).  A dot product of K terms plus a bias, accumulated in fp32 in any order, with or without fused multiply-adds,
has |got - exact| <= gamma_(K+1) S, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms,
(3.5)): K roundings of partial sums / FMAs and one for the bias.  The matrix pipe adds its terms in groups of four whose internal order
and intermediate rounding are not documented: one more rounding per group is covered by doubling.  The references multiply the fp32
operands as stored, except where a packer folds BatchNorm in float64 and rounds once (deconv): one more u S.  Together
(K + 2) u S with the factor 2 for summation order and grouping:  |got - ref| <= 2 (K + 2) 2^-24 S  per element.  ReLU is
1-Lipschitz and maps the exact 0 to 0: it does not increase the error.  K is the NOMINAL length (27 or 9 stem, 147 pe_res, cin head,
th tw cat_vec, taps cin deconv) also where a border leaves fewer terms; S only holds the terms that exist.

THE INPUTS.  tests/test_boundary_cases.py requires that in no case more than 5 % of the elements have a bound below 1e-6 max |ref|,
i.e. S < 8.39 / (K + 2) max |ref|.  For K >= 7 that asks for S to be of the size of the largest output everywhere; for the short dot
products (K = 4: head with cin 4; K = 2: cat_vec 9 x 7 -> 2 x 1; one tap: the 1 x 1 stem) it asks for S above the largest output, which
only inputs whose terms cancel can give.  So: activations are positive with magnitudes in [lo, 1] (masks of the pooling kernels:
negative), weights are sign_out (-1)^(sum of the reduction indices) * magnitude in [lo, 1] * scale, biases are small.  Every window --
whole or clipped by a border -- then holds as many positive as negative terms (+- 1): |ref| stays far below S, S is nearly the same for
every element with the same number of terms.  lo = 0.9 where a dot product can be as short as one or two terms, 0.5 elsewhere.  All 24
mantissa bits of every magnitude are random (synth._sym), neighbouring taps carry opposite signs, every output channel its own
magnitudes: a wrong tap, channel or pixel moves the result by 1e-2 S or more, four orders of magnitude above the bound."""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from i2r_amd import synth
from i2r_amd.pack import Packer

SEED = 23
U32 = 2.0 ** -24
SENTINEL = 7.0       # exactly representable in fp32, bf16 and f16
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
DT_NAME = {0: "fp32", 1: "bf16", 2: "f16"}


def fp32_bound(K, S):
    """2 (K + 2) 2^-24 S: derivation in the module docstring"""
    return 2.0 * (K + 2) * U32 * S


def _u(key, shape):
    return torch.from_numpy(synth._sym(SEED, key, tuple(shape), 1.0).astype(np.float64))


def mags(key, shape, lo, scale=1.0):
    """fp32 magnitudes in [lo, 1] * scale"""
    return ((lo + (1.0 - lo) * 0.5 * (_u(key, shape) + 1.0)) * scale).float()


def signs(key, shape):
    return torch.where(_u(key, shape) < 0, -1.0, 1.0).double()


def sym(key, shape, scale=1.0):
    return (_u(key, shape) * scale).float()


def alt(*dims):
    """(-1)^(i + j + ...) over a block of the given extents, float64"""
    idx = torch.zeros(dims, dtype=torch.int64)
    for k, d in enumerate(dims):
        idx = idx + torch.arange(d).view([d if j == k else 1 for j in range(len(dims))])
    return 1.0 - 2.0 * (idx % 2).double()


def weights(key, cout, red, lo, scale):
    """fp32 [cout, *red]: sign of the output channel * alternating sign over the reduction indices * magnitude"""
    s = signs(key + ".s", (cout,)).view([cout] + [1] * len(red))
    return (s * alt(*red).unsqueeze(0) * mags(key, (cout,) + tuple(red), lo, scale).double()).float()


def select(x, n, n_src, n_valid):
    """the images the n output slots of a launch stand for: slot i reads image min(i mod n_src, n_valid - 1) of x [n_valid, ...],
    horizontally mirrored for i >= n_src (the flip test batched into one forward; slots n_valid .. n_src - 1 are capacity padding)"""
    src = [min(i % n_src, n_valid - 1) for i in range(n)]
    return torch.stack([x[j].flip(-1) if i >= n_src else x[j] for i, j in enumerate(src)])


class Case(types.SimpleNamespace):
    pass


# ---------------------------------------------------------------------------------------------------------------------------------
# stem: 3x3 stride-2 pad-1 conv, cin 1 or 3, + bias + ReLU, NCHW -> NHWC
# ---------------------------------------------------------------------------------------------------------------------------------
STEM_INPUTS = ((1, 1, 1, 1, 1), (3, 5, 7, 3, 3), (2, 37, 29, 2, 2), (2, 8, 2, 1, 1), (8, 21, 33, 4, 3))   # (n, h, w, n_src, n_valid)
STEM_COUTS = (16, 32, 64, 128)
STEM_CASES = [Case(id="stem-c%d-o%d-%dx%dx%d-s%dv%d" % (cin, cout, n, h, w, ns, nv), cin=cin, cout=cout, n=n, h=h, w=w, n_src=ns, n_valid=nv,
                   out_cs=cout + 16, K=9 * cin)
              for cout in STEM_COUTS for cin in (1, 3) for (n, h, w, ns, nv) in STEM_INPUTS]


def stem_kernel(cin, cout, dt):
    """the dispatch of i2r_stem_conv: cout 64 runs on the matrix pipe, every other multiple of 16 on the VALU kernel"""
    assert cout % 16 == 0 and cin in (1, 3) and dt in (0, 1, 2)
    return ("stem_mfma_k<%d, %d>" if cout == 64 else "stem_conv_k<%d, %d>") % (cin, dt)


@functools.lru_cache(maxsize=None)
def stem_tensors(cid):
    """x [n_valid, cin, h, w], w [cout, cin, 3, 3], bias [cout], fp32"""
    c = BY_ID[cid]
    x = mags("stem.x.%d.%d.%d" % (c.cin, c.h, c.w), (c.n_valid, c.cin, c.h, c.w), 0.9)
    w = weights("stem.w.%d.%d" % (c.cin, c.cout), c.cout, (c.cin, 3, 3), 0.9, 0.5)
    b = sym("stem.b.%d" % c.cout, (c.cout,), 0.01)
    return x, w, b


def stem_value(xs, w, b):
    """-> (relu(conv), S) NHWC float64 of already selected images xs [n, cin, h, w]"""
    xs, w, b = xs.double(), w.double(), b.double()
    ref = F.relu(F.conv2d(xs, w, b, 2, 1))
    S = F.conv2d(xs.abs(), w.abs(), b.abs(), 2, 1)
    return ref.permute(0, 2, 3, 1).contiguous(), S.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def stem_reference(cid):
    """(ref, S) float64 [n, oh, ow, cout]; |fp32 kernel - ref| <= fp32_bound(9 cin, S).  The 16-bit outputs are the same call's fp32
    output rounded once to the storage type, bit for bit."""
    c = BY_ID[cid]
    x, w, b = stem_tensors(cid)
    return stem_value(select(x, c.n, c.n_src, c.n_valid), w, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# pe_res_stem: conv_pre (1 -> 3, 3x3, pad 1, no bias), then conv1 (3 -> 64, 7x7, stride 2, pad 3) + bias + ReLU
# ---------------------------------------------------------------------------------------------------------------------------------
PE_RES_SIZES = ((1, 1), (5, 3), (16, 16), (17, 18), (38, 30))
PE_RES_CASES = [Case(id="peres-%dx%d-%s-cs%d" % (h, w, "mirror" if flip else "plain", cs), h=h, w=w, n=4 if flip else 2, n_src=2, n_valid=2,
                     out_cs=cs, K=147) for (h, w) in PE_RES_SIZES for flip in (False, True) for cs in (64, 80)]
PE_RES_CASES.append(Case(id="peres-17x18-mirror-cs80-s3v2", h=17, w=18, n=6, n_src=3, n_valid=2, out_cs=80, K=147))


@functools.lru_cache(maxsize=None)
def pe_res_tensors(cid):
    """mask [n_valid, 1, h, w], w_pre [3, 1, 3, 3], w7 [64, 3, 7, 7] (BatchNorm folded: the kernel's operand), bias [64], fp32"""
    c = BY_ID[cid]
    m = mags("peres.m.%d.%d" % (c.h, c.w), (c.n_valid, 1, c.h, c.w), 0.5)
    return m, weights("peres.pre", 3, (1, 3, 3), 0.5, 0.6), weights("peres.w7", 64, (3, 7, 7), 0.5, 0.2), sym("peres.b", (64,), 0.05)


def pe_res_value(ms, w_pre, w7, b):
    """-> (ref, bound) NHWC float64.  bound = fp32_bound(147, S) + (9 + 2) 2^-24 sum |w7| Spre:  conv_pre's fp32 output is off by at
    most gamma_9 Spre <= (9 + 2) u Spre (Spre = sum |m w_pre|, nine FMAs in one fixed order, no bias: no factor 2), and conv1 carries
    that through |w7| (already BatchNorm-folded here, so the fold's scale factor is in it); S = sum |pre w7| + |bias| of the exact pre."""
    ms, w_pre, w7, b = ms.double(), w_pre.double(), w7.double(), b.double()
    pre = F.conv2d(ms, w_pre, None, 1, 1)
    ref = F.relu(F.conv2d(pre, w7, b, 2, 3))
    S = F.conv2d(pre.abs(), w7.abs(), b.abs(), 2, 3)
    prop = F.conv2d(F.conv2d(ms.abs(), w_pre.abs(), None, 1, 1), w7.abs(), None, 2, 3)
    bound = fp32_bound(147, S) + (9 + 2) * U32 * prop
    return ref.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def pe_res_reference(cid):
    c = BY_ID[cid]
    m, w_pre, w7, b = pe_res_tensors(cid)
    return pe_res_value(select(m, c.n, c.n_src, c.n_valid), w_pre, w7, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# max-pool 3x3 stride 2 pad 1 (padding = -inf), NHWC
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [Case(id="pool-%dx%dx%d-c%d-%d-%d" % (n, h, w, c, ics, ocs), n=n, h=h, w=w, c=c, in_cs=ics, out_cs=ocs)
              for (n, h, w) in ((2, 1, 1), (2, 2, 5), (3, 9, 7), (1, 16, 12)) for (c, ics, ocs) in ((4, 4, 4), (12, 16, 32), (64, 64, 96))]


def negative_map(key, shape, positive=0.15):
    """fp32, magnitudes in [0.1, 1], negative but for a share `positive` of the elements: a max over a window that includes zero
    padding is 0 or a positive element, never the negative maximum of the window's real elements"""
    m = mags(key, shape, 0.1).double()
    return torch.where(_u(key + ".pos", shape) > 1.0 - 2.0 * positive, m, -m).float()


@functools.lru_cache(maxsize=None)
def pool_tensors(cid):
    c = BY_ID[cid]
    return negative_map("pool.%d.%d.%d.%d" % (c.n, c.h, c.w, c.c), (c.n, c.h, c.w, c.c))


def pool_value(x, pad_value=float("-inf")):
    """NHWC float64 max-pool; comparisons are exact, so the fp32 kernel must agree bit for bit"""
    xp = F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1), value=pad_value)
    return F.max_pool2d(xp, 3, 2, 0).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def pool_reference(cid):
    return pool_value(pool_tensors(cid))


# ---------------------------------------------------------------------------------------------------------------------------------
# head: 1x1 conv + bias, NHWC -> NCHW
# ---------------------------------------------------------------------------------------------------------------------------------
HEAD_SIZES = ((1, 1, 5), (3, 9, 7), (1, 6, 6), (2, 4, 8))   # hw = 5 (fewer than 16 pixels), 63 (scalar stores), 36 and 32 (16-byte stores)
HEAD_MFMA = [(cin, cout) for cin in (16, 48, 128) for cout in (1, 16, 17, 32)]
HEAD_VALU = [(cin, cout) for cin in (4, 20, 132, 144) for cout in (1, 16, 17, 20, 21, 32)]
HEAD_WIDE = {(48, 17), (132, 21)}   # one case of each kind whose rows are 16 channels wider than cin
HEAD_CASES = [Case(id="head-%d-%d-%dx%dx%d" % (cin, cout, n, h, w), cin=cin, cout=cout, n=n, h=h, w=w,
                   in_cs=cin + 16 if (cin, cout) in HEAD_WIDE else cin, K=cin)
              for (cin, cout) in HEAD_MFMA + HEAD_VALU for (n, h, w) in HEAD_SIZES]


def head_kernel(cin, cout, hw, npix):
    """the dispatch of i2r_head, and for the matrix-pipe kernel the store path its lanes take"""
    assert cin % 4 == 0 and 1 <= cout <= 32
    if cin % 16 == 0 and cin <= 128 and npix + 256 < 2 ** 31:
        return "head_mfma_k<%d>/%s" % (1 if cout <= 16 else 2, "vector" if hw % 4 == 0 else "scalar")
    return "head_k<%d>" % (16 if cout <= 16 else 20 if cout <= 20 else 32)


def head_lds_bytes(cin, cout):
    """dynamic LDS of the VALU head: [cin / 4][JP] 16-byte weight quadruples"""
    return cin // 4 * (16 if cout <= 16 else 20 if cout <= 20 else 32) * 16


@functools.lru_cache(maxsize=None)
def head_tensors(cid):
    """x [n, h, w, cin], w [cout, cin], bias [cout], fp32"""
    c = BY_ID[cid]
    lo = 0.9 if c.cin < 16 else 0.5
    return (mags("head.x.%d.%d.%d.%d" % (c.cin, c.n, c.h, c.w), (c.n, c.h, c.w, c.cin), lo),
            weights("head.w.%d.%d" % (c.cin, c.cout), c.cout, (c.cin,), lo, 0.2), sym("head.b.%d.%d" % (c.cin, c.cout), (c.cout,), 0.02))


def head_value(x, w, b):
    """-> (ref, S) float64 NCHW"""
    x, w, b = x.double(), w.double(), b.double()
    return F.linear(x, w, b).permute(0, 3, 1, 2).contiguous(), F.linear(x.abs(), w.abs(), b.abs()).permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def head_reference(cid):
    return head_value(*head_tensors(cid))


# ---------------------------------------------------------------------------------------------------------------------------------
# pe_cat_vec: the mask max-pooled `rate` times, flattened, through a linear layer; the vector repeated over the tokens
# ---------------------------------------------------------------------------------------------------------------------------------
CAT_SHAPES = ((50, 44, 2, 13, 11), (9, 7, 3, 2, 1), (3, 5, 0, 3, 5))   # (h, w, rate, th, tw): odd intermediate extents 25 x 22, 5 x 4 / 3 x 2
CAT_CASES = [Case(id="cat-%dx%d-r%d-v%d-c%d" % (h, w, rate, vec, c0), h=h, w=w, rate=rate, th=th, tw=tw, vec=vec, c0=c0, c_end=c0 + vec + 4,
                  out_cs=c0 + vec + 12, n=6, n_src=3, n_valid=2, K=th * tw)
             for (h, w, rate, th, tw) in CAT_SHAPES for vec in (40, 300) for c0 in (0, 78)]


@functools.lru_cache(maxsize=None)
def cat_tensors(cid):
    """mask [n_valid, h, w] (negative; a few positive elements where the dot product is long), wfc [vec, th tw], bfc [vec], fp32"""
    c = BY_ID[cid]
    P = c.th * c.tw
    m = -mags("cat.m.%d.%d" % (c.h, c.w), (c.n_valid, c.h, c.w), 0.9).double()
    m[:, 0] *= 0.93       # the first and the last row hold the largest values: windows that differ only in one of them differ in their maximum
    m[:, -1] *= 0.93      # (9 x 7 pooled three times: rows 0..7 and rows 1..8)
    m = m.float()
    if P >= 64:
        m = torch.where(_u("cat.pos.%d.%d" % (c.h, c.w), m.shape) > 0.94, -m, m)
    return m, weights("cat.w.%d.%d" % (P, c.vec), c.vec, (P,), 0.9, 0.3), sym("cat.b.%d" % c.vec, (c.vec,), 0.01)


def cat_pooled(ms, rate, pad_value=float("-inf")):
    """[n, h, w] -> [n, th tw] float64: `rate` cascaded MaxPool2d(3, 2, 1)"""
    p = ms.double().unsqueeze(1)
    for _ in range(rate):
        p = F.max_pool2d(F.pad(p, (1, 1, 1, 1), value=pad_value), 3, 2, 0)
    return p.flatten(1)


def cat_value(pooled, wfc, bfc):
    """-> (v, S) float64 [n, vec]"""
    return F.linear(pooled, wfc.double(), bfc.double()), F.linear(pooled.abs(), wfc.double().abs(), bfc.double().abs())


@functools.lru_cache(maxsize=None)
def cat_reference(cid):
    """(v, S) [n, vec]: every token row of image i holds v[i] in channels [c0, c0 + vec) and zeros in [c0 + vec, c_end); the pooling is
    exact in fp32, so K = th tw"""
    c = BY_ID[cid]
    m, wfc, bfc = cat_tensors(cid)
    return cat_value(cat_pooled(select(m, c.n, c.n_src, c.n_valid), c.rate), wfc, bfc)


# ---------------------------------------------------------------------------------------------------------------------------------
# fuse_up_add: out = act((base + up(t1)) + up(t2)), nearest-neighbour up-sampling
# ---------------------------------------------------------------------------------------------------------------------------------
FUSE_SCALES = ((2,), (8,), (2, 4), (4, 2), (2, 8))
FUSE_SHAPES = ((3, 8, 8, 4), (2, 24, 8, 48))   # (n, h, w, cs)
FUSE_CASES = [Case(id="fuse-%s-%dx%dx%dx%d-%s" % ("+".join(map(str, sc)), n, h, w, cs, DT_NAME[dt]), scales=sc, n=n, h=h, w=w, cs=cs, dt=dt)
              for sc in FUSE_SCALES for (n, h, w, cs) in FUSE_SHAPES for dt in (0, 1, 2)]


def fuse_kernel(dt):
    return "fuse_up_add_k<%d>" % dt


@functools.lru_cache(maxsize=None)
def fuse_tensors(cid):
    """(base, [terms]) NHWC in the storage type of the case: what the buffers hold.  Three 16-bit numbers of similar size add up exactly
    in fp32, in any order (f16 values below 1 are all multiples of 2^-24: their sums never round at all); so the values spread over 25
    binades up to 64 (sym * 2^(6 - e), e = 0..24, the f16 ones down into the subnormals: then base + t1 does round in fp32), and a quarter
    of the base elements are exactly minus the last term, so that the rounding of the first sum survives the cancellation and the final
    rounding to 16 bit.  Half of the values are negative: the ReLU matters."""
    c = BY_ID[cid]

    def wide(key, shape, e0=0, e1=24):
        e = torch.floor(e0 + 0.5 * (e1 + 1 - e0) * (_u(key + ".e", shape) + 1.0)).clamp(e0, e1)
        return (_u(key, shape) * torch.pow(2.0, 6.0 - e)).float().to(TDT[c.dt])
    tag = "%d.%d.%d" % (c.n, c.h, c.cs)
    two = len(c.scales) == 2   # then the first term is the small one (e = 12..24) and the last the large one (e = 0..12)
    terms = [wide("fuse.t%d.%d.%s" % (i, s, tag), (c.n, c.h // s, c.w // s, c.cs), 12 * (two and i == 0), 24 - 12 * (two and i == 1))
             for i, s in enumerate(c.scales)]
    base = wide("fuse.b." + tag, (c.n, c.h, c.w, c.cs))
    base = torch.where(_u("fuse.m." + tag, base.shape) < -0.5, -up_nearest(terms[-1], c.scales[-1]), base)
    return base, terms


def up_nearest(t, s):
    return t.repeat_interleave(s, 1).repeat_interleave(s, 2)


def fuse_value(base, terms, scales, act, dt, order=(0, 1)):
    """The stored operands widened to fp32 (exact), summed in fp32 in the kernel's order (base + t1) + t2 -- an fp32 addition is
    correctly rounded on either machine, so the order fixes every bit --, ReLU, rounded ONCE to the storage type.  Bit-exact for all
    three storage types; for fp32 storage the last step does nothing."""
    v = base.float()
    ups = [up_nearest(t.float(), s) for t, s in zip(terms, scales)]
    for i in (order if len(ups) == 2 else (0,)):
        v = v + ups[i]
    if act:
        v = F.relu(v)
    return v.to(TDT[dt])


# ---------------------------------------------------------------------------------------------------------------------------------
# deconv: ConvTranspose2d(k, stride 2, padding p, output_padding op) + BatchNorm (+ ReLU) (+ residual after the ReLU)
# ---------------------------------------------------------------------------------------------------------------------------------
DECONV_CFG = {4: (1, 0), 3: (1, 1), 2: (0, 0)}   # k -> (padding, output_padding): _get_deconv_cfg of the reference
DECONV_SHAPES = ((2, 48, 48, 5, 3), (1, 40, 24, 1, 1), (3, 96, 32, 8, 6))   # (n, cin, cout, h, w)
DECONV_CASES = [Case(id="deconv-k%d-%dx%d-%d-%dx%d" % (k, n, cin, cout, h, w), k=k, n=n, cin=cin, cout=cout, h=h, w=w,
                     K=(4 if k > 2 else 1) * cin) for k in (4, 3, 2) for (n, cin, cout, h, w) in DECONV_SHAPES]


@functools.lru_cache(maxsize=None)
def deconv_tensors(cid):
    """x [n, cin, h, w], the state-dict entries of the layer (ConvTranspose2d weight [cin, cout, k, k] + BatchNorm), post [n, cout, 2h, 2w]"""
    c = BY_ID[cid]
    tag = "deconv.%d.%d.%d" % (c.k, c.cin, c.cout)
    w = weights(tag + ".w", c.cout, (c.cin, c.k, c.k), 0.5, 0.1).permute(1, 0, 2, 3).contiguous()
    sd = {"d.weight": w, "b.weight": mags(tag + ".g", (c.cout,), 0.8, 1.2), "b.bias": sym(tag + ".beta", (c.cout,), 0.05),
          "b.running_mean": sym(tag + ".mean", (c.cout,), 0.05), "b.running_var": mags(tag + ".var", (c.cout,), 0.6, 1.4)}
    x = mags(tag + ".x.%d.%d" % (c.h, c.w), (c.n, c.cin, c.h, c.w), 0.5)
    post = sym(tag + ".post.%d.%d" % (c.h, c.w), (c.n, c.cout, 2 * c.h, 2 * c.w), 0.5)
    return x, sd, post


def deconv_folded(sd, eps=1e-5):
    """float64 (w [cin, cout, k, k], bias [cout]) with the eval-mode BatchNorm folded in"""
    scale = sd["b.weight"].double() / torch.sqrt(sd["b.running_var"].double() + eps)
    return sd["d.weight"].double() * scale.view(1, -1, 1, 1), sd["b.bias"].double() - sd["b.running_mean"].double() * scale


@functools.lru_cache(maxsize=None)
def deconv_reference(cid, relu, with_post):
    """(ref, S) float64 NCHW [n, cout, 2h, 2w].  S = sum |x w'| + |b'| (+ |post|: the residual is added after the ReLU, one more
    rounding of a value no larger than S); K = taps * cin with the 4 taps of the fullest parity (k = 2: one tap)."""
    c = BY_ID[cid]
    x, sd, post = deconv_tensors(cid)
    w, b = deconv_folded(sd)
    p, op = DECONV_CFG[c.k]
    ref = F.conv_transpose2d(x.double(), w, b, 2, p, op)
    S = F.conv_transpose2d(x.double().abs(), w.abs(), b.abs(), 2, p, op)
    if relu:
        ref = F.relu(ref)
    if with_post:
        ref, S = ref + post.double(), S + post.double().abs()
    return ref, S


def deconv_by_parity(x, w, b, k, swap=False):
    """The same transposed conv from the per-parity tap formula of Packer.DECONV_TAPS, float64, before ReLU:
    out[2q + py, 2r + px] = b + sum_(dy, dx) in[q + iy0 + dy, r + ix0 + dx] w[:, :, kys[dy], kxs[dx]].  swap: the parities' output offsets
    exchanged (the wrong variant)."""
    n, cin, h, wd = x.shape
    out = torch.zeros(n, w.shape[1], 2 * h, 2 * wd, dtype=torch.float64)
    xp = F.pad(x.double(), (1, 1, 1, 1))
    for py in (0, 1):
        for px in (0, 1):
            (iy0, kys), (ix0, kxs) = Packer.DECONV_TAPS[k][py], Packer.DECONV_TAPS[k][px]
            acc = b.view(1, -1, 1, 1).expand(n, -1, h, wd).clone()
            for dy, ky in enumerate(kys):
                for dx, kx in enumerate(kxs):
                    acc += torch.einsum("nchw,co->nohw", xp[:, :, 1 + iy0 + dy:1 + iy0 + dy + h, 1 + ix0 + dx:1 + ix0 + dx + wd], w[:, :, ky, kx])
            out[:, :, (1 - py if swap else py)::2, (1 - px if swap else px)::2] = acc
    return out


ALL_CASES = STEM_CASES + PE_RES_CASES + POOL_CASES + HEAD_CASES + CAT_CASES + FUSE_CASES + DECONV_CASES
BY_ID = {c.id: c for c in ALL_CASES}
assert len(BY_ID) == len(ALL_CASES)


def ids(cases):
    return [c.id for c in cases]
