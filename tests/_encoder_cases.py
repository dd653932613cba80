"""The fp32 encoder kernels (csrc/i2r_encoder.hip: enc_kv_k, enc_layer4_k) at ragged group edges: the case table, the float64 references
and a harness that drives i2r_encoder_kv / i2r_encoder_layer through the raw C-ABI on poisoned buffers.

Groups are token counts.  The float64 reference is the CPU oracle itself (i2r_cpu.inter_human_encoder is dtype-generic) called with double
tensors on feat [S, d, 1, 1] and length = tokens per group, i.e. one "person" per token; plain_layer is an independent per-group loop the
table checks the padded-and-masked oracle against.  Which kernel a case runs is asked of the library (i2r_encoder_layer_form), never
re-derived here."""
import collections
import ctypes as C
import functools

import torch
import torch.nn.functional as F

import i2r_cpu
from _gpu_util import NAN_WORD
from i2r_amd import cabi, engine, synth

EDGE = [1, 15, 16, 17, 31, 33, 47, 48, 49, 63, 65, 97, 113, 129]   # 724 tokens, 53 tiles, 31 two-tile work items
DIMS = (96, 78)
DFF = 192
POS_MODES = ("none", "rows", "table")
PERIOD = 48                      # pos table rows (token % PERIOD)
TAIL_ROWS = 37                   # token rows behind the last group offset (case tail-rows)
GUARD = 4096                     # floats behind the documented K / V workspace bound
SPLIT_WS_FLOATS = 256 * 2 * 1792
CNT_POISON = 0x01010101          # split_cnt before i2r_encoder_kv: non-zero, the kv launch re-arms the counters

Case = collections.namedtuple("Case", "name lens rot scratch tail shift purpose")


def _c(name, lens, rot, purpose, scratch=True, tail=0, shift=False):
    return Case(name, tuple(lens), rot, scratch, tail, shift, purpose)


# rot: the pos mode of a run is POS_MODES[(rot + (d == 78) + (n_layers == 1)) % 3] -- the cases of one form carry different rot, so every
# (DC, form) pair meets every mode (checked through the query in test_encoder_cases.py).  shift: + 0.75 on the input (token means far from 0).
CASES = collections.OrderedDict((c.name, c) for c in [
    _c("one-edge", EDGE, 0, "one-tile form, 53 tiles, grid 56"),
    _c("one-many", [1, 15, 16, 17] * 20, 1, "80 groups: second trip of locate_tile", shift=True),
    _c("one-big", EDGE * 10, 2, "530 tiles, 310 items: one-tile form above two tiles per CU"),
    _c("split-edge", EDGE * 6, 0, "318 tiles, t_x 40", shift=True),
    _c("split-low", EDGE * 4 + [16] * 45, 1, "257 tiles: t_x 33, slots past n_qblk"),
    _c("split-high", EDGE * 9 + [17] * 12, 2, "501 tiles: t_x 63", shift=True),
    _c("split-short", [5] * 300, 0, "one ragged fragment per group: upper halves without keys"),
    _c("whole-noscratch", EDGE * 6, 0, "split_ws = split_cnt = NULL: one workgroup per tile at 318 tiles", scratch=False, shift=True),
    _c("two-edge", EDGE * 17, 0, "527 items, 238 groups (four trips)"),
    _c("two-threshold-512", EDGE * 16 + [32] * 16, 1, "512 work items: two-tile form", shift=True),
    _c("two-threshold-511", EDGE * 16 + [32] * 15, 1, "511 work items: one-tile form"),
    _c("tail-rows", EDGE, 2, "37 token rows behind the last offset", tail=TAIL_ROWS, shift=True),
])
VARIANTS = [(name, d, nl) for name in CASES for d in DIMS for nl in (3, 1)]


def pos_mode(case, d, n_layers):
    return POS_MODES[(case.rot + (d == 78) + (n_layers == 1)) % 3]


def counts(lens):
    """(n_qtiles16, n_qtiles32, n_qtiles64, n_qtiles192): what the host tells the launcher about the groups"""
    return tuple(sum(-(-n // t) for n in lens) for t in (16, 32, 64, 192))


def offsets(lens):
    o = [0]
    for n in lens:
        o.append(o[-1] + n)
    return o


def _rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(11, key, tuple(shape), scale))


def _encoder_sd(d, dff, tag):
    """one layer's weights, scaled as test_kernels_gpu._encoder_sd scales them"""
    p = "L"
    sd = {p + ".self_attn.in_proj_weight": _rand((3 * d, d), "ipw" + tag, 2.5 * (3.0 / d) ** 0.5),
          p + ".self_attn.in_proj_bias": _rand((3 * d,), "ipb" + tag, 0.1),
          p + ".self_attn.out_proj.weight": _rand((d, d), "opw" + tag, (3.0 / d) ** 0.5),
          p + ".self_attn.out_proj.bias": _rand((d,), "opb" + tag, 0.1),
          p + ".linear1.weight": _rand((dff, d), "l1w" + tag, (3.0 / d) ** 0.5),
          p + ".linear1.bias": _rand((dff,), "l1b" + tag, 0.1),
          p + ".linear2.weight": _rand((d, dff), "l2w" + tag, (3.0 / dff) ** 0.5),
          p + ".linear2.bias": _rand((d,), "l2b" + tag, 0.1)}
    for n in ("norm1", "norm2"):
        sd[p + ".%s.weight" % n] = _rand((d,), n + "w" + tag, 0.3) + 1.0
        sd[p + ".%s.bias" % n] = _rand((d,), n + "b" + tag, 0.2)
    return sd


@functools.lru_cache(maxsize=None)
def layer_weights(d, i):
    """fp32 state dict (keys "L....") of layer i of the width-d stack; every case shares them"""
    return _encoder_sd(d, DFF, "ec%d_%d" % (i, d))


@functools.lru_cache(maxsize=None)
def _stack_sd(d, layers, dtype):
    """the oracle's state dict "E.layers.<j>...." holding the given layers in that order"""
    sd = {}
    for j, i in enumerate(layers):
        sd.update({k.replace("L.", "E.layers.%d." % j): v.to(dtype) for k, v in layer_weights(d, i).items()})
    return sd


@functools.lru_cache(maxsize=None)
def inputs(name, d, n_layers):
    """(src [rows, d], pos [rows, d] as the kernel adds it | None, table [PERIOD, d] | None, mode) of a run, fp32 CPU.  rows = tokens of
    the groups + the case's tail rows; the table form is materialised as table[arange(rows) % PERIOD]."""
    case = CASES[name]
    rows = sum(case.lens) + case.tail
    src = _rand((rows, d), "src%s%d" % (name, d)) + (0.75 if case.shift else 0.0)
    mode = pos_mode(case, d, n_layers)
    pos = table = None
    if mode == "rows":
        pos = _rand((rows, d), "pos%s%d" % (name, d), 0.5)
    elif mode == "table":
        table = _rand((PERIOD, d), "tab%s%d" % (name, d), 0.5)
        pos = table[torch.arange(rows) % PERIOD]
    return src, pos, table, mode


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def _as_feat(t, n, dtype):
    return None if t is None else t[:n].to(dtype).reshape(n, t.shape[1], 1, 1)


def ref_layer(d, i, x, pos, lens, dtype=torch.float64):
    """layer i of the stack applied to the token rows x [>= sum(lens), d] (+ pos rows | None) by the CPU oracle in `dtype` -> [sum(lens), d]"""
    n = sum(lens)
    return i2r_cpu.inter_human_encoder(_stack_sd(d, (i,), dtype), "E", 1, _as_feat(x, n, dtype), _as_feat(pos, n, dtype), list(lens)).reshape(n, d)


def ref_stack(d, n_layers, x, pos, lens, dtype=torch.float64):
    """-> list of the n_layers layer outputs [sum(lens), d] of the oracle stack in `dtype`"""
    n = sum(lens)
    col = {}
    i2r_cpu.inter_human_encoder(_stack_sd(d, tuple(range(n_layers)), dtype), "E", n_layers, _as_feat(x, n, dtype), _as_feat(pos, n, dtype),
                                list(lens), collect=col)
    return [col["E.layers.%d" % i].reshape(n, d) for i in range(n_layers)]


def ref_kv(d, i, x, pos, n, dtype=torch.float64):
    """K = (x + pos) Wk^T + bk and V = x Wv^T + bv of layer i for the first n token rows -> ([n, d], [n, d])"""
    sd = layer_weights(d, i)
    w, b = sd["L.self_attn.in_proj_weight"].to(dtype), sd["L.self_attn.in_proj_bias"].to(dtype)
    xs = x[:n].to(dtype)
    xp = xs if pos is None else xs + pos[:n].to(dtype)
    return F.linear(xp, w[d:2 * d], b[d:2 * d]), F.linear(xs, w[2 * d:], b[2 * d:])


def plain_layer(d, i, x, pos, lens):
    """layer i in float64 as a plain loop over the groups -- softmax(q k^T) v on the group's own rows, no padding, no mask, LayerNorm
    written out -- the independent check of ref_layer's padded-and-masked route"""
    sd = {k: v.double() for k, v in layer_weights(d, i).items()}
    w, b = sd["L.self_attn.in_proj_weight"], sd["L.self_attn.in_proj_bias"]

    def ln(y, n):
        mu = y.mean(-1, keepdim=True)
        var = ((y - mu) ** 2).mean(-1, keepdim=True)
        return (y - mu) / torch.sqrt(var + 1e-5) * sd["L.%s.weight" % n] + sd["L.%s.bias" % n]

    out, o = [], 0
    for n in lens:
        xs = x[o:o + n].double()
        xp = xs if pos is None else xs + pos[o:o + n].double()
        q = (xp @ w[:d].t() + b[:d]) * d ** -0.5
        k = xp @ w[d:2 * d].t() + b[d:2 * d]
        v = xs @ w[2 * d:].t() + b[2 * d:]
        a = torch.softmax(q @ k.t(), -1) @ v
        y = ln(xs + a @ sd["L.self_attn.out_proj.weight"].t() + sd["L.self_attn.out_proj.bias"], "norm1")
        f = torch.relu(y @ sd["L.linear1.weight"].t() + sd["L.linear1.bias"]) @ sd["L.linear2.weight"].t() + sd["L.linear2.bias"]
        out.append(ln(y + f, "norm2"))
        o += n
    return torch.cat(out)


def err_max_rms(a, ref64):
    e = (a.double() - ref64).abs()
    return e.max().item(), e.pow(2).mean().sqrt().item()


# ---------------------------------------------------------------------------------------------------------------------------------
# the fragment-packed K / V^T workspaces
# ---------------------------------------------------------------------------------------------------------------------------------
def unpack_kv(buf, n_frag, cs, vt=False):
    """The first n_frag fragments of a kbuf / vbuf (flat floats) back as matrices: the inverse of engine.pack_frag per fragment.
    vt False: K, the operand image of [16 keys, cs] per fragment -> [n_frag, 16, cs].
    vt True: V, the operand image of V^T [cs dims, 16 keys] per fragment (store_kv_frag) -> V as [n_frag, 16 keys, cs dims] too."""
    dc = cs // 16
    b = buf[:n_frag * 16 * cs]
    if not vt:  # [frag][c][g][li][r] = K[li][16 c + 4 g + r]
        return b.reshape(n_frag, dc, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(n_frag, 16, cs)
    # [frag][rb][g][li][r] = V^T[16 rb + li][4 g + r]
    return b.reshape(n_frag, dc, 4, 16, 4).permute(0, 1, 3, 2, 4).reshape(n_frag, cs, 16).transpose(1, 2)


def key_slots(lens):
    """(frag, row) of every token -- fragments are numbered group by group, 16 keys each -- and the fragment count"""
    frag, row, base = [], [], 0
    for n in lens:
        j = torch.arange(n)
        frag.append(base + j // 16)
        row.append(j % 16)
        base += -(-n // 16)
    return torch.cat(frag), torch.cat(row), base


def kv_floats(n_tok, n_grp, cs):
    """the documented workspace bound (include/i2r_hip.h, fp32 mode)"""
    return (n_tok // 16 + n_grp) * 16 * cs


# ---------------------------------------------------------------------------------------------------------------------------------
# descriptors and the form query
# ---------------------------------------------------------------------------------------------------------------------------------
_PTRS = ("src", "kbuf", "vbuf", "out", "grp_off", "w_in", "b_in", "w_out", "b_out", "ln1_w", "ln1_b", "w1", "b1", "w2", "b2", "ln2_w", "ln2_b")
_LP_PTRS = ("w_in_lp", "w_out_lp", "w1_lp", "w2_lp", "vec_lp")


def set_groups(desc, lens, n_tok=None):
    desc.n_tok, desc.n_grp = (sum(lens) if n_tok is None else n_tok), len(lens)
    desc.n_qtiles16, desc.n_qtiles32, desc.n_qtiles64, desc.n_qtiles192 = counts(lens)
    return desc


def dummy_desc(lens, d=96, scratch=True, dtype=0, pos_period=0):
    """a descriptor the library accepts without a device behind it: distinct non-null dummy pointers (the query launches nothing)"""
    desc = cabi.EncoderDesc()
    for i, n in enumerate(_PTRS + (_LP_PTRS if dtype else ())):
        setattr(desc, n, 0x10000 * (i + 1))
    if scratch:
        desc.split_ws, desc.split_cnt = 0x7000000, 0x7100000
    desc.d, desc.cs, desc.dff_pad, desc.ln_eps, desc.dtype, desc.pos_period = d, (d + 15) // 16 * 16, DFF, 1e-5, dtype, pos_period
    if pos_period:
        desc.pos = 0x7200000
    return set_groups(desc, lens)


def layer_form(desc):
    """(qt, ks, grid) of what i2r_encoder_layer would launch"""
    qt, ks, grid = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    cabi.check(cabi.lib().i2r_encoder_layer_form(C.byref(desc), C.byref(qt), C.byref(ks), C.byref(grid)), "i2r_encoder_layer_form")
    return qt.value, ks.value, grid.value


FORM_NAMES = {(1, 1): "one", (1, 2): "split", (2, 1): "two"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness (device side)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packed_layers(d, n_layers, device):
    return [engine.Packer(layer_weights(d, i), torch.device(device)).encoder_layer("L", d, DFF) for i in range(n_layers)]


Run = collections.namedtuple("Run", "outs snaps")   # outs: per layer [rows, cs] CPU; snaps: per launch dict(k=[2], v=[2], cnt, ws) CPU


class Stack:
    """A kv launch + n_layers layer launches (fused K / V tails on all but the last) over buffers this object owns: src, pos, one out per
    layer, two kbuf / vbuf pairs of exactly the documented size + GUARD, the offset table and the split scratch; descriptors filled the
    way Program.encoder fills them."""

    def __init__(self, lens, d, n_layers, device, src, pos=None, table=None, scratch=True, tail=0):
        self.lens, self.d, self.cs, self.n_layers, self.dev = list(lens), d, (d + 15) // 16 * 16, n_layers, torch.device(device)
        self.n_cov, self.rows = sum(lens), sum(lens) + tail
        assert src.shape == (self.rows, d)
        self.layers = packed_layers(d, n_layers, str(device))
        self.src_host = self._pad(src)
        self.src = self.src_host.to(self.dev)
        self.pos = None
        if table is not None:
            self.pos = self._pad(table).to(self.dev)
        elif pos is not None:
            self.pos = self._pad(pos).to(self.dev)
        self.kv_used = counts(lens)[0] * 16 * self.cs
        self.kv_size = kv_floats(self.rows, len(lens), self.cs)
        assert self.kv_used <= self.kv_size
        new = lambda n: torch.empty(n, dtype=torch.float32, device=self.dev)
        self.outs = [new(self.rows * self.cs).view(self.rows, self.cs) for _ in range(n_layers)]
        self.kbufs, self.vbufs = [new(self.kv_size + GUARD) for _ in range(2)], [new(self.kv_size + GUARD) for _ in range(2)]
        self.goff = torch.tensor(offsets(lens), dtype=torch.int32, device=self.dev)
        self.split_ws = new(SPLIT_WS_FLOATS) if scratch else None
        self.split_cnt = torch.empty(256, dtype=torch.int32, device=self.dev) if scratch else None
        self.descs = []
        for i, L in enumerate(self.layers):
            desc = cabi.EncoderDesc()
            desc.src = (self.src if i == 0 else self.outs[i - 1]).data_ptr()
            desc.pos = self.pos.data_ptr() if self.pos is not None else None
            desc.kbuf, desc.vbuf, desc.out, desc.grp_off = self.kbufs[i % 2].data_ptr(), self.vbufs[i % 2].data_ptr(), self.outs[i].data_ptr(), self.goff.data_ptr()
            for name in ("w_in", "b_in", "w_out", "b_out", "ln1_w", "ln1_b", "w1", "b1", "w2", "b2", "ln2_w", "ln2_b"):
                setattr(desc, name, L[name].data_ptr())
            desc.d, desc.cs, desc.dff_pad, desc.ln_eps = d, self.cs, L["dff_pad"], 1e-5
            desc.pos_period = PERIOD if table is not None else 0
            if scratch:
                desc.split_ws, desc.split_cnt = self.split_ws.data_ptr(), self.split_cnt.data_ptr()
            if i + 1 < n_layers:
                nxt = self.layers[i + 1]
                desc.next_w_in, desc.next_b_in = nxt["w_in"].data_ptr(), nxt["b_in"].data_ptr()
                desc.next_kbuf, desc.next_vbuf = self.kbufs[(i + 1) % 2].data_ptr(), self.vbufs[(i + 1) % 2].data_ptr()
            self.descs.append(set_groups(desc, lens, self.rows))
        self.form = layer_form(self.descs[0])
        assert all(layer_form(x) == self.form for x in self.descs)

    def _pad(self, t):
        o = torch.zeros(t.shape[0], self.cs)
        o[:, :self.d] = t
        return o

    def workspaces(self):
        return self.outs + self.kbufs + self.vbufs + ([self.split_ws] if self.split_ws is not None else [])

    def poison(self):
        for t in self.workspaces():
            t.view(torch.int32).fill_(NAN_WORD)
        if self.split_cnt is not None:
            self.split_cnt.fill_(CNT_POISON)

    def load_src(self, host=None):
        """src poisoned, then loaded again (host: other token rows, padded here)"""
        self.src.view(torch.int32).fill_(NAN_WORD)
        self.src.copy_(self.src_host if host is None else self._pad(host))

    def _snap(self):
        s = dict(k=[t.clone() for t in self.kbufs], v=[t.clone() for t in self.vbufs])
        s["cnt"] = self.split_cnt.clone() if self.split_cnt is not None else None
        return s

    def run(self, poison=True):
        """kv + the layers on the current stream; a stream-ordered copy of the workspaces and counters is taken behind every launch"""
        L, st = cabi.lib(), torch.cuda.current_stream().cuda_stream
        if poison:
            self.poison()
        cabi.check(L.i2r_encoder_kv(C.byref(self.descs[0]), st), "i2r_encoder_kv")
        snaps = [self._snap()]
        for desc in self.descs:
            cabi.check(L.i2r_encoder_layer(C.byref(desc), st), "i2r_encoder_layer")
            snaps.append(self._snap())
        torch.cuda.synchronize()
        ws = self.split_ws.cpu() if self.split_ws is not None else None
        snaps = [dict(k=[t.cpu() for t in s["k"]], v=[t.cpu() for t in s["v"]], cnt=None if s["cnt"] is None else s["cnt"].cpu(), ws=ws) for s in snaps]
        return Run([o.cpu() for o in self.outs], snaps)


def is_poison(t):
    return bool((t.view(torch.int32) == NAN_WORD).all())
