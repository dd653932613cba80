"""Cases and float64 references for the fp32 HRFormer-B path: the four glue kernels of csrc/i2r_hrformer.hip (i2r_layernorm,
i2r_window_attn, i2r_dwconv3x3, i2r_upsample_bilinear_add(_multi)) and the block / module emitters on top of them
(engine.HRFormerB._emit_block, ._emit_module).

Every case names the edge it is there for.  tests/test_hrformer_cases.py checks on the CPU that a table hits the edges it claims (by
mirroring the launch arithmetic of the host wrappers), that the loop-form window attention below is the oracle's, and that the plain
fp32 torch restatement of every case stays within a quarter of the case's tolerance against float64 (well-conditioned inputs: the
tolerance is not what makes a case pass).  tests/test_hrformer_fp32_gpu.py runs every case on the GPU against the float64 value.

Nothing here calls into csrc/ for the expected values.  Kernel-level references are float64 torch; block and module references are
the dtype-generic oracle (oracle/i2r_cpu_hrformer.py) run on a .double() state dict.  Weights come from arch.Spec +
arch_hrformer._transformer_block / _module + synth.make_state_dict.

Tolerances (max-abs) are the project's own for the same operation, never the kernel's result:
  LayerNorm 2e-5 (test_layernorm), dwconv 5e-5 (test_dwconv), upsample one term 1e-5 (test_upsample_bilinear_add), several terms 2e-5
  (test_upsample_bilinear_add_several_terms_in_one_pass), window attention and blocks 2e-4 (test_window_attention_block_matches_oracle),
  modules 1e-3 (the tower-level bound of tests/test_model_gpu.py); 16-bit storage: the float64 value rounded once, 1 ulp of the
  storage type (2^-8 bf16 / 2^-11 f16, relative) + 1e-5 (test_layernorm_and_dwconv_16bit_storage)."""
import collections
import functools

import torch
import torch.nn.functional as F

import i2r_cpu_hrformer as H
from i2r_amd import arch, arch_hrformer, synth
from i2r_amd.pack import _r16

TOL_LN, TOL_DW, TOL_UP1, TOL_UPN, TOL_ATTN, TOL_BLOCK, TOL_MODULE = 2e-5, 5e-5, 1e-5, 2e-5, 2e-4, 2e-4, 1e-3
ULP = {1: 2.0 ** -8, 2: 2.0 ** -11}
TDT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}
HP = 40       # head pitch of i2r_window_attn (Packer.HEAD_PAD)
WINDOW = 7
SEED = 11


def rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(SEED, "hrf." + key, tuple(shape), scale))


# ------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------------------------
LnCase = collections.namedtuple("LnCase", "id edge n c h w shift out_dt")
LN_CASES = [
    LnCase("c17", "cs 48 of 17: one chunk mixes real and pad channels, the rest are whole pad chunks", 3, 17, 9, 7, 0.0, 0),
    LnCase("c78", "cs 80: 20 chunks, lanes 4..15 idle in the second round", 3, 78, 9, 7, 0.0, 0),
    LnCase("c312", "cs 320: five full rounds", 3, 312, 9, 7, 0.0, 0),
    LnCase("c624", "cs == c: no pad channel", 3, 624, 9, 7, 0.0, 0),
    LnCase("c640", "the limit: all ten register chunks of every lane", 3, 640, 9, 7, 0.0, 0),
    LnCase("npix1", "one pixel: 15 of 16 pixel groups of the workgroup idle", 1, 78, 1, 1, 0.0, 0),
    LnCase("npix15", "15 pixels: one short of a workgroup", 3, 78, 1, 5, 0.0, 0),
    LnCase("npix17", "17 pixels: one into the second workgroup", 1, 78, 1, 17, 0.0, 0),
    LnCase("shift8", "mean 8 against a spread of 2: the variance is taken about the mean", 3, 312, 9, 7, 8.0, 0),
    LnCase("c78_bf16", "bf16 output, pad channels stored as 16-bit zeros", 3, 78, 9, 7, 0.0, 1),
    LnCase("c78_f16", "f16 output", 3, 78, 9, 7, 0.0, 2),
    LnCase("c624_bf16", "bf16 output, cs == c", 3, 624, 9, 7, 0.0, 1),
    LnCase("c624_f16", "f16 output, cs == c", 3, 624, 9, 7, 0.0, 2),
]


def ln_launch(case):
    """the arithmetic of i2r_layernorm / layernorm_k: 16 lanes per pixel, 16 pixels per workgroup, 10 float4 chunks per lane"""
    cs = _r16(case.c)
    npix = case.n * case.h * case.w
    return dict(cs=cs, nch=cs // 4, npix=npix, blocks=(npix * 16 + 255) // 256, rounds=-(-(cs // 4) // 16),
                mixed=[ch for ch in range(cs // 4) if ch * 4 < case.c < ch * 4 + 4], pad_chunks=[ch for ch in range(cs // 4) if ch * 4 >= case.c])


def ln_tensors(case):
    c = case.c
    x = rand((case.n, c, case.h, case.w), "ln.x." + case.id, 2.0) + case.shift
    return x, rand((c,), "ln.w." + case.id, 0.3) + 1.0, rand((c,), "ln.b." + case.id, 0.2)


def ln_ref(x, w, b, eps=1e-6):
    """LayerNorm over c of an NCHW map, in the dtype of x (float64: the reference)"""
    t = x.permute(0, 2, 3, 1)
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (((t - mu) / torch.sqrt(var + eps)) * w + b).permute(0, 3, 1, 2)


def ln_fp32(x, w, b):
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, 1e-6).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------------------
# window attention (kernel level: q/k/v already projected, in the kernel's layout)
# ------------------------------------------------------------------------------------------------------------------------------
WaCase = collections.namedtuple("WaCase", "id edge n heads hd h w qscale")
_WA_HEADS = [(2, 39), (4, 39), (16, 39), (2, 40), (2, 37), (4, 38)]
_WA_MAPS = [(7, 7, "one whole window, no padding"), (1, 2, "smaller than a window: pad 3+3 rows, 2+3 columns"),
            (5, 9, "pad 1+1 rows; two windows across, pad 2+3 columns"), (13, 3, "two windows down, pad 0+1 rows; pad 2+2 columns"),
            (8, 15, "padded both ways: 2x3 windows, 3+3 pad rows and 3+3 pad columns"), (14, 21, "six whole windows")]
WA_CASES = ([WaCase("h%dx%d_5x9" % (hh, hd), "head width %d, %d heads%s" % (hd, hh, "" if hd == 39 else " (accepted: hd in 37..40)"), 3, hh, hd, 5, 9, 1.0)
             for hh, hd in _WA_HEADS]
            + [WaCase("h2x39_%dx%d" % (h, w), e, 3, 2, 39, h, w, 1.0) for h, w, e in _WA_MAPS if (h, w) != (5, 9)]
            + [WaCase("h4x38_8x15", "narrow head on the asymmetric map", 3, 4, 38, 8, 15, 1.0),
               WaCase("h2x39_9x8", "odd padding: 5 rows (2 before, 3 after), 6 columns", 3, 2, 39, 9, 8, 1.0),
               WaCase("h2x39_8x15_spread", "scores spread to about +-30 (q scaled by 5): max-subtraction and exp over a wide range", 3, 2, 39, 8, 15, 5.0)])


def wa_launch(case):
    """the arithmetic of i2r_window_attn"""
    nwy, nwx = (case.h + 6) // 7, (case.w + 6) // 7
    ph, pw = nwy * 7 - case.h, nwx * 7 - case.w
    return dict(nwy=nwy, nwx=nwx, pad_top=ph // 2, pad_bottom=ph - ph // 2, pad_left=pw // 2, pad_right=pw - pw // 2,
                blocks=case.n * nwy * nwx * case.heads, hs=case.heads * HP, c=case.heads * case.hd)


def wa_tensors(case):
    """qkv [n, h, w, 3*hs] and the bias vector [3*hs] in the kernel's layout: head hh at channels hh*40 .. hh*40 + hd - 1 of each part,
    the pad dims exactly zero"""
    hs = case.heads * HP
    real = torch.zeros(3 * hs, dtype=torch.bool)
    for part in range(3):
        for hh in range(case.heads):
            real[part * hs + hh * HP: part * hs + hh * HP + case.hd] = True
    qkv = rand((case.n, case.h, case.w, 3 * hs), "wa.qkv." + case.id)
    bias = rand((3 * hs,), "wa.bias." + case.id, 0.5)
    qkv[..., :hs] *= case.qscale
    bias[:hs] *= case.qscale
    return qkv * real, bias * real


def window_attention_loop(qkv, bias, heads, hd):
    """Independent loop form of the 7x7-window attention over already projected q | k | v, in the dtype of qkv: windows and heads one by
    one.  The map is centre-padded to whole windows (pad // 2 before); a border token's q, k and v are the bias vector (the projection of
    a zero input); border tokens are ordinary keys, and their queries are dropped.  -> [n, h, w, heads*40], pad dims zero."""
    n, h, w, _ = qkv.shape
    hs = heads * HP
    nwy, nwx = -(-h // WINDOW), -(-w // WINDOW)
    pad_top, pad_left = (nwy * WINDOW - h) // 2, (nwx * WINDOW - w) // 2
    out = torch.zeros(n, h, w, hs, dtype=qkv.dtype)
    for img in range(n):
        for wy in range(nwy):
            for wx in range(nwx):
                pos = [(wy * WINDOW + ty - pad_top, wx * WINDOW + tx - pad_left) for ty in range(WINDOW) for tx in range(WINDOW)]
                inside = [0 <= y < h and 0 <= x < w for y, x in pos]
                tok = torch.stack([qkv[img, y, x] if ok else bias for (y, x), ok in zip(pos, inside)])   # [49, 3*hs]
                for hh in range(heads):
                    q, k, v = (tok[:, part * hs + hh * HP: part * hs + hh * HP + hd] for part in range(3))
                    o = torch.softmax(q @ k.t(), dim=-1) @ v
                    for t, ((y, x), ok) in enumerate(zip(pos, inside)):
                        if ok:
                            out[img, y, x, hh * HP: hh * HP + hd] = o[t]
    return out


def project_qkv(sd, p, x, heads):
    """x [n, h, w, c] -> (qkv, bias) in the kernel's layout with the oracle's projection weights (hd^-0.5 folded into q), dtype of x"""
    c = x.shape[-1]
    hd, hs = c // heads, heads * HP
    qkv = torch.zeros(*x.shape[:3], 3 * hs, dtype=x.dtype)
    bias = torch.zeros(3 * hs, dtype=x.dtype)
    for part, name in enumerate(("q_proj", "k_proj", "v_proj")):
        sc = float(hd) ** -0.5 if part == 0 else 1.0
        y = F.linear(x, sd["%s.%s.weight" % (p, name)], sd["%s.%s.bias" % (p, name)]) * sc
        for hh in range(heads):
            qkv[..., part * hs + hh * HP: part * hs + hh * HP + hd] = y[..., hh * hd:(hh + 1) * hd]
            bias[part * hs + hh * HP: part * hs + hh * HP + hd] = sd["%s.%s.bias" % (p, name)][hh * hd:(hh + 1) * hd] * sc
    return qkv, bias


def unpad_heads(a, heads, hd):
    """[..., heads*40] -> [..., heads*hd]"""
    return torch.cat([a[..., hh * HP: hh * HP + hd] for hh in range(heads)], -1)


# ------------------------------------------------------------------------------------------------------------------------------
# depth-wise 3x3 conv
# ------------------------------------------------------------------------------------------------------------------------------
DwCase = collections.namedtuple("DwCase", "id edge n c h w stride act bias bn dt")
_STRIP = {1: "a column shorter than one 4-row strip", 2: "half a strip", 3: "one row short of a strip", 5: "one row into the second strip",
          9: "two strips and one row"}
DW_CASES = ([DwCase("s1_%dx%d" % (h, w), _STRIP[h] + (", one column: no horizontal neighbour" if w == 1 else ""), 3, 78, h, w, 1, 2, True, True, 0)
             for h in (1, 2, 3, 5, 9) for w in (1, 7)]
            + [DwCase("s1_c1248_5x7", "the hidden width of the 312 branch, cs == c", 3, 1248, 5, 7, 1, 2, True, True, 0),
               DwCase("s1_c1248_1x1", "cs == c on a single pixel", 3, 1248, 1, 1, 1, 2, True, True, 0)]
            + [DwCase("s1_act%d_%s" % (act, "bb" if full else "plain"), "act %d, %s" % (act, "bias and BN" if full else "neither bias nor BN"),
                      3, 78, 5, 7, 1, act, full, full, 0) for act in (0, 1, 2) for full in (False, True)]
            + [DwCase("s1_%s_h%d" % ("bf16" if dt == 1 else "f16", h), "16-bit storage of input and output, %s" % _STRIP[h], 3, 312, h, 7, 1, 2, True,
                      False, dt) for dt in (1, 2) for h in (5, 9)]
            + [DwCase("s2_c%d_%dx%d" % (c, h, w), e, 3, c, h, w, 2, 0, False, c == 78, 0)
               for c in (78, 156) for h, w, e in ((1, 1, "stride 2 on one pixel: only the centre tap"), (2, 3, "even rows, odd columns -> 1x2"),
                                                  (7, 5, "odd both ways -> 4x3, last taps past the map"), (8, 6, "even both ways -> 4x3"))])


def dw_launch(case):
    """the arithmetic of i2r_dwconv3x3"""
    cs = _r16(case.c)
    out_h, out_w = (case.h - 1) // case.stride + 1, (case.w - 1) // case.stride + 1
    strips = (case.h + 3) // 4
    nthr = case.n * strips * case.w * (cs // 4) if case.stride == 1 else case.n * out_h * out_w * (cs // 4)
    return dict(cs=cs, out_h=out_h, out_w=out_w, strips=strips, tail_rows=case.h % 4, nthr=nthr, blocks=(nthr + 255) // 256)


def dw_tensors(case):
    """-> (x, state dict with d.weight [, d.bias] [, b.*])"""
    c = case.c
    sd = {"d.weight": rand((c, 1, 3, 3), "dw.w." + case.id, 0.5)}
    if case.bias:
        sd["d.bias"] = rand((c,), "dw.b." + case.id, 0.2)
    if case.bn:
        sd.update({"b.weight": rand((c,), "dw.g." + case.id, 0.5) + 1.0, "b.bias": rand((c,), "dw.bb." + case.id, 0.3),
                   "b.running_mean": rand((c,), "dw.m." + case.id, 0.3), "b.running_var": rand((c,), "dw.v." + case.id, 0.4) + 1.0})
    x = rand((case.n, c, case.h, case.w), "dw.x." + case.id)
    if case.dt:
        x = x.to(TDT[case.dt]).float()  # (the stored input is the rounded one)
    return x, sd


def act_ref(y, act):
    return F.gelu(y) if act == 2 else F.relu(y) if act == 1 else y


def dw_ref(x, sd, stride, act):
    """depth-wise 3x3 (pad 1) [+ bias] [+ eval-mode BN] + activation in the dtype of x"""
    cast = {k: v.to(x.dtype) for k, v in sd.items()}
    y = F.conv2d(x, cast["d.weight"], cast.get("d.bias"), stride=stride, padding=1, groups=x.shape[1])
    if "b.weight" in cast:
        sh = (1, -1, 1, 1)
        y = (y - cast["b.running_mean"].view(sh)) / torch.sqrt(cast["b.running_var"].view(sh) + 1e-5) * cast["b.weight"].view(sh) + cast["b.bias"].view(sh)
    return act_ref(y, act)


# ------------------------------------------------------------------------------------------------------------------------------
# bilinear up-sample + accumulate
# ------------------------------------------------------------------------------------------------------------------------------
UpCase = collections.namedtuple("UpCase", "id edge n c H W scales act alias")
_LOW = {(1, 1): "1x1 low map: both clamps at once", (1, 3): "one low row: y1 clamps to y0 everywhere", (3, 1): "one low column",
        (3, 5): "interior and all four borders"}
UP_CASES = ([UpCase("x%d_%dx%d" % (s, lh, lw), _LOW[(lh, lw)], 3, 78, lh * s, lw * s, (s,), 1, False) for s in (2, 4, 8) for (lh, lw) in _LOW]
            + [UpCase("m" + "_".join(map(str, sc)), "%d terms in one pass on 16x8%s" % (len(sc), ": the 1/8 map is 2x1" if 8 in sc else ""), 3, 78, 16, 8, sc, 1,
                      False) for sc in ((2, 2), (4, 2), (2, 4, 8), (8, 4, 2))]
            + [UpCase("x2_3x5_act0", "no activation", 3, 78, 6, 10, (2,), 0, False), UpCase("x2_3x5_act2", "GELU in the up-sample pass", 3, 78, 6, 10, (2,), 2, False),
               UpCase("m2_4_8_act0", "three terms, no activation", 3, 78, 16, 8, (2, 4, 8), 0, False),
               UpCase("m2_4_8_act2", "three terms, GELU", 3, 78, 16, 8, (2, 4, 8), 2, False),
               UpCase("x2_3x5_alias", "res is out: every thread reads its own pixel before it writes it", 3, 78, 6, 10, (2,), 1, True),
               UpCase("m4_2_alias", "two terms, res is out", 3, 78, 16, 8, (4, 2), 1, True),
               UpCase("x4_c624", "cs == c", 3, 624, 4, 12, (4,), 1, False)])


def up_tol(case):
    return TOL_UP1 if len(case.scales) == 1 else TOL_UPN


def up_launch(case):
    cs = _r16(case.c)
    nthr = case.n * case.H * case.W * (cs // 4)
    return dict(cs=cs, nthr=nthr, blocks=(nthr + 255) // 256, lows=[(case.H // s, case.W // s) for s in case.scales])


def up_tensors(case):
    res = rand((case.n, case.c, case.H, case.W), "up.r." + case.id)
    lows = [rand((case.n, case.c, case.H // s, case.W // s), "up.l%d." % i + case.id) for i, s in enumerate(case.scales)]
    return res, lows


def bilinear_term(low, s, H, W):
    """up-sampling by the integer factor s, align_corners=False, as upsample_add_k forms one term: src = max((dst + 0.5) / s - 0.5, 0),
    neighbours clamped to the last row / column, hy * (hx v00 + lx v01) + ly * (hx v10 + lx v11)"""
    lh, lw = low.shape[2:]
    assert (lh * s, lw * s) == (H, W)

    def axis(n_out, n_low):
        src = ((torch.arange(n_out, dtype=low.dtype) + 0.5) / s - 0.5).clamp(min=0)
        i0 = src.floor().long()
        i1 = i0 + (i0 < n_low - 1).long()
        l1 = src - i0.to(low.dtype)
        return i0, i1, l1, 1 - l1
    y0, y1, ly, hy = axis(H, lh)
    x0, x1, lx, hx = axis(W, lw)
    ly, hy = ly.view(-1, 1), hy.view(-1, 1)
    v00, v01, v10, v11 = low[:, :, y0][..., x0], low[:, :, y0][..., x1], low[:, :, y1][..., x0], low[:, :, y1][..., x1]
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)


def up_ref(res, lows, scales, act):
    """act(((res + up(l0)) + up(l1)) + up(l2)) in the kernel's term order, dtype of res"""
    r = res
    for low, s in zip(lows, scales):
        r = r + bilinear_term(low, s, res.shape[2], res.shape[3])
    return act_ref(r, act)


def up_fp32(res, lows, scales, act):
    r = res
    for low, s in zip(lows, scales):
        r = r + F.interpolate(low, scale_factor=s, mode="bilinear", align_corners=False)
    return act_ref(r, act)


# ------------------------------------------------------------------------------------------------------------------------------
# blocks and modules
# ------------------------------------------------------------------------------------------------------------------------------
BlockCase = collections.namedtuple("BlockCase", "id edge n c heads h w")
BLOCK_CASES = [
    BlockCase("c78_5x9", "pad 1+1 rows, two windows across", 2, 78, 2, 5, 9),
    BlockCase("c78_15x8", "three windows down with 3+3 pad rows, 3+3 pad columns; 15 rows = 3 strips + 3", 2, 78, 2, 15, 8),
    BlockCase("c156_7x7", "one whole window", 2, 156, 4, 7, 7),
    BlockCase("c312_13x3", "narrow map, 1248 hidden channels", 2, 312, 8, 13, 3),
    BlockCase("c624_1x2", "the lowest branch at its smallest: two pixels per crop", 2, 624, 16, 1, 2),
    BlockCase("c624_8x6", "the lowest branch at the workload's size", 2, 624, 16, 8, 6),
]
ModuleCase = collections.namedtuple("ModuleCase", "id edge n nb h w blocks multiscale mods")
MODULE_CASES = [
    ModuleCase("nb2_10x6", "two branches; the lower one is 5x3", 2, 2, 10, 6, 1, True, 1),
    ModuleCase("nb3_12x20", "three branches: one fused up-sample pass of two terms, a two-hop down path", 2, 3, 12, 20, 1, True, 1),
    ModuleCase("nb4_16x8", "four branches: three up-sample terms in one pass, early first terms; the lowest branch is 2x1", 2, 4, 16, 8, 1, True, 1),
    ModuleCase("nb4_8x16", "the lowest branch is 1x2", 2, 4, 8, 16, 1, True, 1),
    ModuleCase("nb4_16x8_single", "multiscale=False: one output, two blocks per branch", 2, 4, 16, 8, 2, False, 1),
    ModuleCase("nb3_12x20_chain", "two modules in one fork region, as the modules of a stage: the second one's blocks take over the buffers the first one "
               "handed back through release_deferred / all_waited", 2, 3, 12, 20, 1, True, 2),
]
_CH, _HEADS = (78, 156, 312, 624), (2, 4, 8, 16)


def block_stage(case):
    return dict(num_branches=1, num_channels=(case.c,), num_blocks=(1,), num_heads=(case.heads,))


def module_stage(case):
    return dict(num_branches=case.nb, num_channels=_CH[:case.nb], num_blocks=(case.blocks,) * case.nb, num_heads=_HEADS[:case.nb])


def module_state_dict(st, multiscale, mods=1):
    """weights of `mods` consecutive modules under the key prefixes m, m1, m2, ..."""
    spec = arch.Spec()
    for q in module_keys(mods):
        arch_hrformer._module(spec, q, st, multiscale)
    return synth.make_state_dict(spec, seed=SEED)


def module_keys(mods):
    return ["m" if k == 0 else "m%d" % k for k in range(mods)]


def _double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def _err(a, b):
    return (a.double() - b.double()).abs().max().item()


@functools.lru_cache(maxsize=None)
def block_reference(case):
    """-> (state dict, stage dict, x, float64 reference, max-abs error of the fp32 oracle against it); computed once, shared, never modified"""
    st = block_stage(case)
    sd = module_state_dict(st, True)
    x = rand((case.n, case.c, case.h, case.w), "blk.x." + case.id, 1.7)
    ref = H.transformer_block(_double(sd), "m.branches.0.0", x.double(), case.heads)
    return sd, st, x, ref, _err(H.transformer_block(sd, "m.branches.0.0", x, case.heads), ref)


@functools.lru_cache(maxsize=None)
def module_reference(case):
    """-> (state dict, stage dict, inputs, float64 references, max-abs error of the fp32 oracle against them)"""
    st = module_stage(case)
    sd = module_state_dict(st, case.multiscale, case.mods)
    xs = [rand((case.n, _CH[i], case.h >> i, case.w >> i), "mod.x%d." % i + case.id, 1.7) for i in range(case.nb)]
    sd64 = _double(sd)
    refs, got = [x.double() for x in xs], xs
    for q in module_keys(case.mods):
        refs = H.hr_transformer_module(sd64, q, refs, st, case.multiscale)
        got = H.hr_transformer_module(sd, q, got, st, case.multiscale)
    return sd, st, xs, refs, max(_err(a, b) for a, b in zip(got, refs))


ALL_TABLES = (LN_CASES, WA_CASES, DW_CASES, UP_CASES, BLOCK_CASES, MODULE_CASES)


def storage_bound(ref, dt):
    """element-wise bound of a 16-bit stored result: the float64 value rounded once"""
    return ULP[dt] * ref.abs() + 1e-5


def report(group, case_id, gpu_err, fp32_err, tol):
    """one line of the per-case error table (GPU against float64 next to fp32 torch against float64)"""
    print("HRF-ERR %-8s %-22s gpu %.3e  fp32-torch %.3e  bound %.1e" % (group, case_id, gpu_err, fp32_err, tol))
