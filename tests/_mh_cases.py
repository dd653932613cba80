"""Multi-head attention (csrc/i2r_encoder_mh.hip: enc_mh_attn_k<HB, NQ>, entry point i2r_mh_attention) at ragged group edges: the case
table, the inputs, the float64 reference and a harness that drives the entry point through the raw C-ABI on poisoned buffers.

Every case names the edge it is there for.  Which kernel a case runs is asked of the library (i2r_mh_attention_form, which launches
nothing), never re-derived here; tests/test_mh_cases.py checks on the CPU that the table reaches all 24 instantiations and every
workgroup shape, that the loop reference below is the oracle's attention, that fp32 restatements stay within a quarter of the tolerance
(the tolerance is not what makes a case pass) and that wrong variants differ by 50 x the tolerance.  tests/test_mh_attention_gpu.py runs
every case on the GPU.  Nothing here calls into csrc/ or engine.Program for an expected value.

Inputs (synth._sym: all mantissa bits random): v uniform in [-1, 1], k of unit variance, q of unit variance times scale * hd^-0.5 (the host
folds head_dim^-0.5 into q; scale 3 = logits of a few units), the pad dims hd..hp of q, k and v exactly 0.  The "rising" variant sorts each
group's keys by the score of the group's first query, so that query's running maximum grows with every key tile and every tile rescales
its accumulator; it runs at scale 6, and only at hp <= 48 (test_mh_cases.py: beyond that fp32 itself leaves the quarter).

TOL is the project's own bar for this operation at unit-scale v (test_kernels_gpu.py::test_mh_attention_*), never the kernel's result."""
import collections
import ctypes as C
import functools
import math

import torch

from _encoder_cases import EDGE, counts, offsets
from _gpu_util import NAN_WORD
from i2r_amd import cabi, synth

TOL = 2e-5
SEED = 11
TAIL_ROWS = 37          # token rows behind the last group offset (case tail-rows)
GUARD_ROWS = 3          # rows of `out` in front of and behind the launch's rows
MIN_WAVES = 4096        # the documented break of the launcher's rule (include/i2r_hip.h); the cases are built around it, the kernel each
#                         one runs is still asked of the library

NQ1_HB, NQ2_HB, NQ4_HB = range(1, 17), range(1, 7), range(1, 3)
INSTANTIATIONS = {(hb, 1) for hb in NQ1_HB} | {(hb, 2) for hb in NQ2_HB} | {(hb, 4) for hb in NQ4_HB}

Case = collections.namedtuple("Case", "name hp hd heads lens scale rising gaps key_len tail nq purpose")
# gaps = (k_off - hs, qk_cs - k_off - hs, v_cs - hs, out_cs - hs); key_len: None | "cycle" | "clamp"; nq: the query tiles per wave the
# case is there for (asserted through the form query)


def _c(name, hp, heads, lens, nq, purpose, hd=None, scale=3.0, rising=False, gaps=(0, 0, 0, 0), key_len=None, tail=0):
    hd = hp - 3 if hd is None else hd
    assert hp % 16 == 0 and hp - 16 < hd <= hp and (hp > 16 or hd in (12, 13, 16))
    assert scale == 3.0 or (rising and scale == 6.0 and hp <= 48)
    return Case(name, hp, hd, heads, tuple(lens), scale, rising, gaps, key_len, tail, nq, purpose)


_HEADS = (1, 2, 3, 4, 8, 5, 6, 7)   # wpb = heads | full blocks | a last block with 1, 2, 3 live waves
_GAPS = lambda out_gap: (8, 12, 4, out_gap)
_cases = [_c("w%d-h%d" % (16 * hb, _HEADS[(hb - 1) % 8]), 16 * hb, _HEADS[(hb - 1) % 8], EDGE, 1,
             "<%d,1> at %d heads: every group and tile edge on 16-query tiles" % (hb, _HEADS[(hb - 1) % 8]), hd=12 if hb == 1 else None)
          for hb in NQ1_HB]
_cases += [_c("n2-w%d" % (16 * hb), 16 * hb, 16, EDGE * 9, 2, "<%d,2>: 279 32-query tiles x 16 heads; short groups leave the second tile clamped" % hb,
              hd=13 if hb == 1 else None) for hb in NQ2_HB]
_cases += [_c("n4-w%d" % (16 * hb), 16 * hb, 16, EDGE * 15, 4, "<%d,4>: 285 64-query tiles x 16 heads; tiles two to four mostly clamped rows" % hb,
              hd=16 if hb == 1 else None) for hb in NQ4_HB]
_cases += [
    _c("t4-4096", 32, 16, EDGE * 13 + [64] * 9, 4, "256 64-query tiles x 16 heads = 4096 waves: the first launch on <2,4>"),
    _c("t4-4095", 32, 15, EDGE * 14 + [64] * 7, 2, "273 64-query tiles x 15 heads = 4095 waves: still <2,2>; last block of three waves"),
    _c("t2-4096", 96, 16, EDGE * 8 + [32] * 8, 2, "256 32-query tiles x 16 heads = 4096 waves: the first launch on <6,2>"),
    _c("t2-4095", 96, 15, EDGE * 8 + [32] * 25, 1, "273 32-query tiles x 15 heads = 4095 waves: still <6,1>"),
    _c("t2-4096-w48", 48, 16, EDGE * 8 + [32] * 8, 2, "the same break at the narrow end of the 32-query range: <3,2>"),
    _c("t2-4095-w48", 48, 15, EDGE * 8 + [32] * 25, 1, "and its other side: <3,1>"),
    _c("far-w112", 112, 16, EDGE * 9, 1, "7632 waves, both counts past the break: heads of 112 dims stay on <7,1>"),
    _c("many-n4", 16, 16, [1, 15, 16, 17] * 80, 4, "320 groups much shorter than the 64-query tile: the grp_off walk at <1,4>", hd=13),
    _c("rise-n1", 48, 3, EDGE, 1, "keys sorted by query 0's score: every key tile rescales o (<3,1>)", scale=6.0, rising=True),
    _c("rise-n2", 32, 16, EDGE * 9, 2, "rising keys at <2,2>", scale=6.0, rising=True),
    _c("rise-n4", 16, 16, EDGE * 15, 4, "rising keys at <1,4>", hd=12, scale=6.0, rising=True),
    _c("st-n1-h1", 80, 1, EDGE, 1, "gaps in every row stride, one head; 4 pad columns behind the heads: lane group 0 only", gaps=_GAPS(4)),
    _c("st-n1-h5", 32, 5, EDGE, 1, "gaps, five heads (a last block of one wave); 12 pad columns: lane groups 0..2", gaps=_GAPS(12)),
    _c("st-n2", 64, 16, EDGE * 9, 2, "gaps at <4,2>; 20 pad columns: all four lane groups and a second trip", gaps=_GAPS(20)),
    _c("st-n4", 32, 16, EDGE * 15, 4, "gaps at <2,4>; 36 pad columns: three trips", gaps=_GAPS(36)),
    _c("kl-n1", 48, 6, EDGE * 6, 1, "key_len cycling 1, len, len - 1, 16, 17, len // 2 over every EDGE length (<3,1>)", key_len="cycle"),
    _c("kl-n2", 80, 16, EDGE * 9, 2, "key_len at <5,2>: the queries past the keys fill whole clamped tiles", key_len="cycle"),
    _c("kl-n4", 16, 16, EDGE * 15, 4, "key_len at <1,4>", hd=12, key_len="cycle"),
    _c("kl-clamp", 32, 3, EDGE * 3, 1, "key_len 0, -5 and len + 7: the documented clamp to [1, len]", key_len="clamp"),
    _c("tail-rows", 32, 7, EDGE, 1, "37 NaN token rows behind the last offset; a last block of three waves", tail=TAIL_ROWS),
]
CASES = collections.OrderedDict((c.name, c) for c in _cases)
assert len(CASES) == len(_cases)


def key_lens(case):
    """the key_len array as the host passes it (unclamped) | None"""
    if case.key_len is None:
        return None
    if case.key_len == "cycle":
        return [min(max((1, n, n - 1, 16, 17, n // 2)[key_len_pattern(i, 6)], 1), n) for i, n in enumerate(case.lens)]   # inside the precondition
    return [(0, -5, n + 7)[key_len_pattern(i, 3)] for i, n in enumerate(case.lens)]


def key_len_pattern(i, n_patterns):
    """which key_len pattern group i carries: one further with every repetition of EDGE, so every length meets every pattern"""
    return (i % len(EDGE) + i // len(EDGE)) % n_patterns


def clamped(klens, lens):
    """what the kernel documents: key_len clamped to [1, group length]"""
    return list(lens) if klens is None else [min(max(kl, 1), n) for kl, n in zip(klens, lens)]


def strides(case):
    """(hs, k_off, qk_cs, v_cs, out_cs)"""
    hs = case.heads * case.hp
    gk, gqk, gv, go = case.gaps
    return hs, hs + gk, hs + gk + hs + gqk, hs + gv, hs + go


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def _rand(shape, key, half_width):
    return torch.from_numpy(synth._sym(SEED, "mh." + key, tuple(shape), half_width))


@functools.lru_cache(maxsize=2)
def inputs(name):
    """(q, k, v) fp32 CPU [n_tok, heads, hp] as the kernel reads them (q scaled, pad dims exactly 0); n_tok = the rows of the groups"""
    case = CASES[name]
    n, H, hp, hd = sum(case.lens), case.heads, case.hp, case.hd
    q, k, v = (torch.zeros(n, H, hp) for _ in range(3))
    q[..., :hd] = _rand((n, H, hd), "q." + name, 3.0 ** 0.5) * (case.scale * hd ** -0.5)
    k[..., :hd] = _rand((n, H, hd), "k." + name, 3.0 ** 0.5)
    v[..., :hd] = _rand((n, H, hd), "v." + name, 1.0)
    if case.rising:
        o = 0
        for L in case.lens:   # keys of the group in the order of query 0's score, per head
            s0 = torch.einsum("hd,khd->hk", q[o].double(), k[o:o + L].double())
            order = s0.argsort(dim=1).t()                                         # [L, H]
            k[o:o + L] = torch.gather(k[o:o + L], 0, order[:, :, None].expand(L, H, hp))
            o += L
    return q, k, v


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def loop_reference(q, k, v, lens, klens=None):
    """THE reference: per group and head, float64 softmax(q k[:kl]^T) v[:kl] of the operands as given, kl = the clamped key_len, as a
    plain loop.  q, k, v [n_tok, heads, hp] -> float64 [n_tok, heads, hp]"""
    q, k, v = (t.double().transpose(0, 1).contiguous() for t in (q, k, v))   # [heads, n_tok, hp]: one head's rows side by side
    out = torch.zeros(q.shape, dtype=torch.float64)
    g0 = 0
    for n, kl in zip(lens, clamped(klens, lens)):
        for h in range(q.shape[0]):
            qq, kk, vv = q[h, g0:g0 + n], k[h, g0:g0 + kl], v[h, g0:g0 + kl]
            out[h, g0:g0 + n] = torch.softmax(qq @ kk.t(), dim=-1) @ vv
        g0 += n
    return out.transpose(0, 1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 [n_tok, heads, hd] of a case, computed once and shared"""
    case = CASES[name]
    q, k, v = inputs(name)
    return loop_reference(q, k, v, case.lens, key_lens(case))[..., :case.hd].contiguous()


def batched(q, k, v, lens, klens=None, dtype=torch.float64, key_rows=None, v_rows=None):
    """The same attention with the heads as a batch dimension, in `dtype` (float32: the plain torch restatement).  key_rows / v_rows
    (g0, n, kl) -> absolute row indices of the group's keys and of their values: the hooks of the wrong variants below."""
    out = torch.zeros(q.shape, dtype=dtype)
    g0 = 0
    for n, kl in zip(lens, clamped(klens, lens)):
        kr = torch.arange(g0, g0 + kl) if key_rows is None else key_rows(g0, n, kl)
        vr = kr if v_rows is None else v_rows(g0, n, kl)
        qq, kk, vv = (t.to(dtype).transpose(0, 1) for t in (q[g0:g0 + n], k[kr], v[vr]))
        out[g0:g0 + n] = (torch.softmax(qq @ kk.transpose(1, 2), dim=-1) @ vv).transpose(0, 1)
        g0 += n
    return out


def online(q, k, v, lens, klens=None, dtype=torch.float32, rescale=True):
    """The kernel's order in `dtype`: exp2 domain (q times log2 e, rounded), key tiles of 16, running maximum m and sum l, o rescaled by
    exp2(m - m_new) before every tile's P V, one division at the end.  rescale=False: the wrong variant that forgets o's rescale."""
    out = torch.zeros(q.shape, dtype=dtype)
    log2e = torch.tensor(1.4426950408889634, dtype=dtype)
    g0 = 0
    for n, kl in zip(lens, clamped(klens, lens)):
        qq = q[g0:g0 + n].to(dtype).transpose(0, 1) * log2e
        m = torch.full(qq.shape[:2], -math.inf, dtype=dtype)
        l, o = torch.zeros_like(m), torch.zeros_like(qq)
        for k0 in range(g0, g0 + kl, 16):
            k1 = min(k0 + 16, g0 + kl)
            s = qq @ k[k0:k1].to(dtype).permute(1, 2, 0)
            m_new = torch.maximum(m, s.max(-1).values)
            alpha, p = torch.exp2(m - m_new), torch.exp2(s - m_new[..., None])
            l, m = l * alpha + p.sum(-1), m_new
            o = (o * alpha[..., None] if rescale else o) + p @ v[k0:k1].to(dtype).transpose(0, 1)
        out[g0:g0 + n] = (o / l[..., None]).transpose(0, 1)
        g0 += n
    return out


# ---- wrong variants, all in float64: what a subtly broken kernel would compute --------------------------------------------------
def _m_drop_last(case, q, k, v, klens):
    return batched(q, k, v, case.lens, klens, key_rows=lambda g0, n, kl: torch.arange(g0, g0 + max(kl - 1, 1)))


def _m_admit_next(case, q, k, v, klens):
    last = q.shape[0] - 1   # (the last group has no successor: it keeps its own keys)
    return batched(q, k, v, case.lens, klens,
                   key_rows=lambda g0, n, kl: torch.cat([torch.arange(g0, g0 + kl), torch.arange(g0 + n, g0 + n + 1)]) if g0 + n <= last else torch.arange(g0, g0 + kl))


def _m_v_shift(case, q, k, v, klens):
    def v_rows(g0, n, kl):
        r, t = torch.arange(g0, g0 + kl), min(16, kl)
        r[:t] = r[:t].roll(1)
        return r
    return batched(q, k, v, case.lens, klens, v_rows=v_rows)


def _m_no_rescale(case, q, k, v, klens):
    return online(q, k, v, case.lens, klens, torch.float64, rescale=False)


def _m_heads_swapped(case, q, k, v, klens):
    o = batched(q, k, v, case.lens, klens)
    o[:, [0, case.heads - 1]] = o[:, [case.heads - 1, 0]]
    return o


def _m_key_len_ignored(case, q, k, v, klens):
    return batched(q, k, v, case.lens, None)


def _m_key_len_on_queries(case, q, k, v, klens):
    o, g0 = batched(q, k, v, case.lens, klens), 0
    for n, kl in zip(case.lens, clamped(klens, case.lens)):
        o[g0 + kl:g0 + n] = 0.0
        g0 += n
    return o


def _m_key_len_unclamped(case, q, k, v, klens):
    """key_len as given: no key at all (an all-zero row), or keys from the next groups' rows"""
    n_tok = q.shape[0]
    o = batched(q, k, v, case.lens, [max(kl, 1) for kl in klens], key_rows=lambda g0, n, kl: torch.arange(g0, min(g0 + kl, n_tok)))
    g0 = 0
    for n, kl in zip(case.lens, klens):
        if kl <= 0:
            o[g0:g0 + n] = 0.0
        g0 += n
    return o


# name -> (variant, the cases it applies to)
MUTANTS = collections.OrderedDict([
    ("last key dropped", (_m_drop_last, lambda c: True)),
    ("first key of the next group admitted", (_m_admit_next, lambda c: True)),
    ("V rows of one 16-key tile shifted by one", (_m_v_shift, lambda c: True)),
    ("rescale of o omitted", (_m_no_rescale, lambda c: c.rising)),
    ("two heads swapped", (_m_heads_swapped, lambda c: c.heads >= 2)),
    ("key_len ignored", (_m_key_len_ignored, lambda c: c.key_len == "cycle")),
    ("key_len applied to the queries too", (_m_key_len_on_queries, lambda c: c.key_len == "cycle")),
    ("key_len not clamped", (_m_key_len_unclamped, lambda c: c.key_len == "clamp")),
])


# ---------------------------------------------------------------------------------------------------------------------------------
# arguments and the form query
# ---------------------------------------------------------------------------------------------------------------------------------
def args_for(case, qk=0x10000, v=0x20000, out=0x30000, grp_off=0x40000, key_len=0x50000):
    """the MhAttnArgs of a case; the default pointers are distinct non-null dummies (the query launches nothing)"""
    hs, k_off, qk_cs, v_cs, out_cs = strides(case)
    n16, n32, n64 = counts(case.lens)[:3]
    return cabi.MhAttnArgs(qk, v, out, grp_off, len(case.lens), case.heads, case.hp, k_off, qk_cs, v_cs, out_cs, n16, n32, n64,
                           key_len if case.key_len else None)


Form = collections.namedtuple("Form", "hb nq grid block")


def form(a):
    """what i2r_mh_attention would launch for these arguments: enc_mh_attn_k<hb, nq>, grid (x, y), threads per workgroup"""
    hb, nq, block, grid = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), (C.c_int32 * 2)(-1, -1)
    cabi.check(cabi.lib().i2r_mh_attention_form(C.byref(a), C.byref(hb), C.byref(nq), grid, C.byref(block)), "i2r_mh_attention_form")
    return Form(hb.value, nq.value, (grid[0], grid[1]), block.value)


def block_shape(heads):
    """(waves per workgroup, live waves of the last workgroup) as include/i2r_hip.h documents them: one wave per head, at most four"""
    wpb = min(heads, 4)
    return wpb, heads - (-(-heads // wpb) - 1) * wpb


# ---------------------------------------------------------------------------------------------------------------------------------
# the harness (device side)
# ---------------------------------------------------------------------------------------------------------------------------------
def is_poison(t):
    return bool((t.contiguous().view(torch.int32) == NAN_WORD).all())


class Launch:
    """One i2r_mh_attention launch of a case over buffers this object owns.  Everything the kernel must not read is NaN: the columns of
    the stride gaps, the token rows behind the last group, and with key_len the k and v parts of every row that is not a key (the q
    part stays: every row is a query).  `out` holds NAN_WORD everywhere before every launch, GUARD_ROWS rows in front and behind
    included."""

    def __init__(self, name, device):
        self.case = case = CASES[name]
        self.dev = torch.device(device)
        hs, k_off, qk_cs, v_cs, out_cs = strides(case)
        self.n_tok = n = sum(case.lens)
        self.rows = rows = n + case.tail
        q, k, v = inputs(name)
        qk = torch.full((rows, qk_cs), math.nan)
        vb = torch.full((rows, v_cs), math.nan)
        qk[:n, :hs], qk[:n, k_off:k_off + hs], vb[:n, :hs] = q.reshape(n, hs), k.reshape(n, hs), v.reshape(n, hs)
        self.klens = key_lens(case)
        if self.klens is not None:
            g0 = 0
            for L, kl in zip(case.lens, clamped(self.klens, case.lens)):
                qk[g0 + kl:g0 + L, k_off:k_off + hs] = math.nan
                vb[g0 + kl:g0 + L] = math.nan
                g0 += L
        self.qk, self.v = qk.to(self.dev), vb.to(self.dev)
        self.out = torch.empty(rows + 2 * GUARD_ROWS, out_cs, dtype=torch.float32, device=self.dev)
        self.goff = torch.tensor(offsets(case.lens), dtype=torch.int32, device=self.dev)
        self.kl = torch.tensor(self.klens, dtype=torch.int32, device=self.dev) if self.klens is not None else None
        self.args = args_for(case, self.qk.data_ptr(), self.v.data_ptr(), self.out[GUARD_ROWS:].data_ptr(), self.goff.data_ptr(),
                             self.kl.data_ptr() if self.kl is not None else None)
        self.form = form(self.args)

    def run(self):
        """poison, launch on the current stream, -> the whole of `out` (guard rows included) on the CPU"""
        self.out.view(torch.int32).fill_(NAN_WORD)
        cabi.check(cabi.lib().i2r_mh_attention(C.byref(self.args), torch.cuda.current_stream().cuda_stream), "i2r_mh_attention")
        torch.cuda.synchronize()
        return self.out.cpu()
