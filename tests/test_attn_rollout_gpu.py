"""-m gpu: the attention roll-out on the MI355X -- the raw i2r_attn_rollout_step C-ABI (chains of steps on both sides, per-person seeds,
up-sampling, canaries, bad arguments) against the float64 product of tests/_attn_rollout_ref.py and against i2r_attn_query_maps /
i2r_attn_person_maps, and net.rollout_at / net.person_rollout against the float64 chain of the restated maps (tests/_attn_ref.py), of
the maps the forward hooks get, and against net.attention_at / net.person_relations.
The bar of a chain of n steps is n x 1e-5 max-abs.  For side 1 (X P^T) that is derived: rows of P sum to 1, so a step does not expand the
max-abs error it is handed and adds at most one map's error (1e-5, the bar of tests/test_attn_maps_gpu.py) times max |X| <= 1.  For side 0
(X P) a step is non-expansive only in the per-row L1 norm, so there n x 1e-5 is a CONVENTION, not a bound.
Every test prints the figures it asserts on (pytest -s).  Measured on the MI355X (max-abs): raw chains of 1 / 2 / 6 steps against float64
5.6e-7 at most on either side, per-person seeds 3.9e-7, one step at alpha 1 against i2r_attn_query_maps 0 and against i2r_attn_person_maps
1.2e-7, up-sampled 1.1e-7; through the model against the restatement's chain 1.2e-5 (bar 1e-3), one layer at alpha 1 against
attention_at 0 / person_relations 7.8e-7, bf16 against the chain of the same model's hook maps 2.7e-6."""
import ctypes
import functools

import pytest
import torch

import _attn_rollout_ref as ref
from _attn_ref import restate
from _golden import setup
from i2r_amd import cabi, models

pytestmark = pytest.mark.gpu
TOL = ref.BAR
TOL_MODEL = 1e-3  # the bar of the hook tests against the CPU restatement
CANARY = 12345.0
N_LAYERS = 6


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _err(got, want):
    return (got.double() - want.to(got.device)).abs().max().item() if want.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# raw C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
class _Job:
    """the tables of one case: groups of lens[g] tokens from token row `start`, one more group behind them that n_grp excludes, and the
    q|k rows of N_LAYERS layers"""

    def __init__(self, lens, start, heads, hp, case):
        self.lens, self.heads, self.hp, self.n_grp = list(lens), heads, hp, len(lens)
        self.offs = [start]
        for n in self.lens + [24]:
            self.offs.append(self.offs[-1] + n)
        layers = [ref.make_qk(heads, hp, self.offs[-1], ref.layer_seed(heads, hp, case, l)) for l in range(N_LAYERS)]
        self.qk = [q.cuda() for q, _, _ in layers]
        self.k_off, self.qk_cs = layers[0][1:]
        self.goff = torch.tensor(self.offs, dtype=torch.int32, device="cuda")
        self.host_off = (ctypes.c_int32 * (self.n_grp + 1))(*self.offs[:self.n_grp + 1])
        self.stride = 2 * heads * max(-(-n // 128) for n in self.lens)
        self.ws = torch.empty(self.stride * self.offs[self.n_grp], device="cuda")

    @functools.cached_property
    def full(self):
        """per layer, per computed group: the float64 [L, L] map on the device (None for an empty group)"""
        return [[ref.full_map(q[o:o + n], self.heads, self.hp, self.k_off) if n else None for o, n in zip(self.offs, self.lens)] for q in self.qk]

    def args(self, layer, src, dst, x_off, side, alpha, K=1, q_cnt=None, seg=0, scale=1, h=1, w=1, out_off=None, rows=None):
        return cabi.AttnRolloutArgs(qk=self.qk[layer].data_ptr(), in_=src.data_ptr(), out=dst.data_ptr(), grp_off=self.goff.data_ptr(), x_off=x_off.data_ptr(),
                                    out_off=out_off.data_ptr() if out_off is not None else None, ws=self.ws.data_ptr(),
                                    q_cnt=q_cnt.data_ptr() if q_cnt is not None else None, rows=rows.data_ptr() if rows is not None else None,
                                    grp_off_host=ctypes.cast(self.host_off, ctypes.c_void_p), n_grp=self.n_grp, heads=self.heads, hp=self.hp,
                                    k_off=self.k_off, qk_cs=self.qk_cs, ws_stride=self.stride, K=K, seg=seg, side=side, scale=scale, h=h, w=w, alpha=alpha)

    def chain(self, seeds, layers, side, alpha, K=1, cnt=None, seg=0, scale=1, h=1, w=1, first=7, gap=5):
        """seeds: per group the fp32 [K_g, L_g] seed (CPU); layers: the layer of every step, in the order the steps run.  Ping-pong between
        two canary-filled buffers; the last step up-samples by `scale`.  Every float outside the computed blocks must keep the canary.
        -> per group the final block (flat)"""
        rows_g = [s.shape[0] for s in seeds]
        offs, pos = [], first
        for r, n in zip(rows_g, self.lens):
            offs.append(pos)
            pos += r * n + gap
        bufs = [torch.full((pos + 32,), CANARY, device="cuda") for _ in range(2)]
        inside = torch.zeros(pos + 32, dtype=torch.bool, device="cuda")
        for o, r, n, s in zip(offs, rows_g, self.lens, seeds):
            inside[o:o + r * n] = True
            bufs[0][o:o + r * n] = s.reshape(-1).cuda()
        x_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        q_cnt = torch.tensor(cnt, dtype=torch.int32, device="cuda") if cnt is not None else None
        Kr = max(rows_g) if seg else K
        for i, layer in enumerate(layers):
            src, dst = bufs[i % 2], bufs[(i + 1) % 2]
            last = i == len(layers) - 1
            if last and scale > 1:
                s2 = scale * scale
                o_offs, opos = [], 4
                for r, n in zip(rows_g, self.lens):
                    o_offs.append(opos)
                    opos += r * n * s2 + gap
                big = torch.full((opos + 32,), CANARY, device="cuda")
                need = Kr * self.offs[self.n_grp]
                rows = torch.full((need + 8,), CANARY, device="cuda")
                before = dst.clone()
                d_ooff = torch.tensor(o_offs, dtype=torch.int64, device="cuda")
                a = self.args(layer, src, big, x_off, side, alpha, K, q_cnt, seg, scale, h, w, d_ooff, rows)
                cabi.check(cabi.lib().i2r_attn_rollout_step(ctypes.byref(a), _stream()), "i2r_attn_rollout_step")
                torch.cuda.synchronize()
                assert (rows[need:] == CANARY).all(), "a store behind the rows workspace"
                assert torch.equal(dst, before), "the up-sampling step wrote the other working buffer"
                wr = torch.zeros(big.numel(), dtype=torch.bool, device="cuda")
                for o, r, n in zip(o_offs, rows_g, self.lens):
                    wr[o:o + r * n * s2] = True
                assert (big[~wr] == CANARY).all(), "a store outside the computed up-sampled blocks"
                assert not (big[wr] == CANARY).any(), "an up-sampled entry was not written"
                return [big[o:o + r * n * s2] for o, r, n in zip(o_offs, rows_g, self.lens)]
            keep = src.clone()
            a = self.args(layer, src, dst, x_off, side, alpha, K, q_cnt, seg)
            cabi.check(cabi.lib().i2r_attn_rollout_step(ctypes.byref(a), _stream()), "i2r_attn_rollout_step")
            torch.cuda.synchronize()
            assert torch.equal(src, keep), "a step wrote its input"
            assert (dst[~inside] == CANARY).all(), "a store outside the computed blocks"
            assert not (dst[inside] == CANARY).any(), "an entry was not written"
        out = bufs[len(layers) % 2]
        return [out[o:o + r * n] for o, r, n in zip(offs, rows_g, self.lens)]


def _layers_of(steps, side):
    """a chain over layers 0 .. steps - 1: side 0 runs hi -> lo, side 1 lo -> hi"""
    return list(range(steps - 1, -1, -1)) if side == 0 else list(range(steps))


@pytest.mark.parametrize("heads,hp", ref.HEADS_HP)
def test_raw_rows_and_columns_at_query_tokens_match_float64(heads, hp):
    job = _Job(ref.QUERY_LENS, ref.QUERY_START, heads, hp, 0)
    worst = {}
    for ki, (K, cnt) in enumerate(ref.QUERY_K):
        tok = ref.query_tokens(K, job.lens, 31 * K + heads)
        used = cnt or [K] * job.n_grp
        seeds = [ref.seed_points(tok[g, :used[g]], n, torch.float32) for g, n in enumerate(job.lens)]
        for steps, alpha in ref.CHAINS:
            T = [ref.rollout([job.full[l][g] for l in range(steps)], alpha) if n else None for g, n in enumerate(job.lens)]
            for side in (0, 1):
                kw = dict(K=K, cnt=cnt, first=7 + ki)
                got = job.chain(seeds, _layers_of(steps, side), side, alpha, **kw)
                again = job.chain(seeds, _layers_of(steps, side), side, alpha, **kw)
                for g, n in enumerate(job.lens):
                    assert torch.equal(got[g], again[g]), "two identical calls differ"
                    if n == 0 or used[g] == 0:
                        assert got[g].numel() == 0
                        continue
                    if alpha == 0.0:
                        assert torch.equal(got[g].cpu(), seeds[g].reshape(-1)), "alpha = 0 must return the seed bit for bit"
                    want = ref.at_tokens(T[g], tok[g, :used[g]], side)
                    e = _err(got[g].view(used[g], n), want)
                    worst[(side, steps)] = max(worst.get((side, steps), 0.0), e)
                    assert e <= steps * TOL, "heads=%d hp=%d K=%d side %d, %d steps alpha %g, group %d: max-abs %.2e" % (heads, hp, K, side, steps, alpha, g, e)
                    neg = [k for k in range(used[g]) if int(tok[g, k]) < 0]
                    assert not got[g].view(used[g], n)[neg].any(), "a zero row of in must give a zero row of out"
    print("heads=%d hp=%d: max-abs vs float64 by (side, steps): %s" % (heads, hp, {k: "%.2e" % v for k, v in sorted(worst.items())}))


@pytest.mark.parametrize("heads,hp", ref.HEADS_HP)
def test_raw_person_seeds_give_dependency_affect_and_relation(heads, hp):
    worst = {}
    for ci, (seg, pers, start) in enumerate(ref.PERSON_CASES):
        job = _Job([p * seg for p in pers], start, heads, hp, 1 + ci)
        for steps, alpha in ref.CHAINS:
            red = [ref.reduce_persons(ref.rollout([job.full[l][g] for l in range(steps)], alpha), seg) if n else None for g, n in enumerate(job.lens)]
            for side in (0, 1):
                seeds = [ref.seed_persons(p, seg, side, torch.float32) for p in pers]
                got = job.chain(seeds, _layers_of(steps, side), side, alpha, seg=seg, first=8 if side else 7, gap=4 if side else 5)
                for g, p in enumerate(pers):
                    if p == 0:
                        assert got[g].numel() == 0
                        continue
                    D, Fm, R, _ = red[g]
                    rows = got[g].view(p, p * seg)
                    e = max(_err(rows, D if side == 0 else Fm), _err(ref.relation_from(rows.double(), seg, side), R))
                    sums = (rows.double().sum(1) - 1).abs().max().item() if side == 0 else (rows.double().sum(0) - 1).abs().max().item()
                    worst[(side, steps)] = max(worst.get((side, steps), 0.0), e, sums)
                    assert max(e, sums) <= steps * TOL, "heads=%d hp=%d seg=%d side %d, %d steps alpha %g, group %d: max-abs %.2e, sums %.2e" % (
                        heads, hp, seg, side, steps, alpha, g, e, sums)
                    if alpha == 0.0:
                        assert torch.equal(rows.cpu(), seeds[g])
    print("heads=%d hp=%d: per-person max-abs vs float64 by (side, steps): %s" % (heads, hp, {k: "%.2e" % v for k, v in sorted(worst.items())}))


def test_raw_one_step_at_alpha_one_is_the_single_layer_forms():
    """one step at alpha = 1 from one-hot seeds = i2r_attn_query_maps (modes 0 and 1); from the person seeds = i2r_attn_person_maps (D, F, R)"""
    heads, hp, K = 2, 48, 17
    job = _Job(ref.QUERY_LENS, ref.QUERY_START, heads, hp, 0)
    tok = ref.query_tokens(K, job.lens, 5)
    seeds = [ref.seed_points(tok[g], n, torch.float32) for g, n in enumerate(job.lens)]
    d_tok = tok.cuda()
    for mode in (0, 1):
        got = job.chain(seeds, [2], mode, 1.0, K=K)
        offs, pos = [], 0
        for n in job.lens:
            offs.append(pos)
            pos += K * n
        out = torch.zeros(pos, device="cuda")
        ws = torch.empty(job.stride * max(job.n_grp * K, job.offs[job.n_grp]), device="cuda")
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
        a = cabi.AttnQueryArgs(qk=job.qk[2].data_ptr(), out=out.data_ptr(), grp_off=job.goff.data_ptr(), out_off=d_off.data_ptr(),
                               ws=ws.data_ptr(), q_tok=d_tok.data_ptr(), n_grp=job.n_grp, heads=heads, hp=hp, k_off=job.k_off, qk_cs=job.qk_cs,
                               n_tiles=sum(-(-K // 16) * -(-n // 128) for n in job.lens) if mode == 0 else sum(-(-n // 16) * -(-n // 128) for n in job.lens),
                               ws_stride=job.stride, mode=mode, K=K, scale=1, h=1, w=1, n_col_tiles=sum(-(-n // 16) * -(-K // 16) for n in job.lens))
        cabi.check(cabi.lib().i2r_attn_query_maps(ctypes.byref(a), _stream()), "i2r_attn_query_maps")
        torch.cuda.synchronize()
        e = max(_err(got[g], out[o:o + K * n].double()) for g, (o, n) in enumerate(zip(offs, job.lens)))
        print("mode %d: one step at alpha 1 vs i2r_attn_query_maps: max-abs %.2e" % (mode, e))
        assert e <= TOL
    for ci, (seg, pers, start) in enumerate(ref.PERSON_CASES):
        job = _Job([p * seg for p in pers], start, heads, hp, 1 + ci)
        n_tok = job.offs[job.n_grp]
        for mode in (1, 2):
            side = mode - 1
            got = job.chain([ref.seed_persons(p, seg, side, torch.float32) for p in pers], [1], side, 1.0, seg=seg)
            r_off, m_off, rpos, mpos = [], [], 0, 0
            for p in pers:
                r_off.append(rpos)
                m_off.append(mpos)
                rpos += p * p
                mpos += p * p * seg
            rel, maps = torch.zeros(rpos, device="cuda"), torch.zeros(mpos, device="cuda")
            rows = torch.zeros(max(pers) * n_tok, device="cuda")
            ws = torch.empty(job.stride * n_tok, device="cuda")
            d_roff, d_moff = torch.tensor(r_off, dtype=torch.int64, device="cuda"), torch.tensor(m_off, dtype=torch.int64, device="cuda")
            a = cabi.AttnPersonArgs(qk=job.qk[1].data_ptr(), grp_off=job.goff.data_ptr(), ws=ws.data_ptr(), rel=rel.data_ptr(),
                                    rel_off=d_roff.data_ptr(), maps=maps.data_ptr(), maps_off=d_moff.data_ptr(), rows=rows.data_ptr(),
                                    grp_off_host=ctypes.cast(job.host_off, ctypes.c_void_p), n_grp=job.n_grp, heads=heads, hp=hp, k_off=job.k_off,
                                    qk_cs=job.qk_cs, ws_stride=job.stride, seg=seg, mode=mode, scale=1, h=1, w=1)
            cabi.check(cabi.lib().i2r_attn_person_maps(ctypes.byref(a), _stream()), "i2r_attn_person_maps")
            torch.cuda.synchronize()
            for g, p in enumerate(pers):
                if p == 0:
                    continue
                rows_g = got[g].view(p, p * seg)
                e = max(_err(rows_g, maps[m_off[g]:m_off[g] + p * p * seg].view(p, p * seg).double()),
                        _err(ref.relation_from(rows_g.double(), seg, side), rel[r_off[g]:r_off[g] + p * p].view(p, p).double()))
                print("seg %d mode %d group %d: one step at alpha 1 vs i2r_attn_person_maps: max-abs %.2e" % (seg, mode, g, e))
                assert e <= TOL


@pytest.mark.parametrize("scale", [2, 4])
def test_raw_upsampling_matches_float64_interpolate(scale):
    h, w, heads, hp, K = 4, 3, 2, 48, 5
    job = _Job([12, 0, 36, 24], 0, heads, hp, 9)
    tok = ref.query_tokens(K, job.lens, 3)
    cnt = [5, 5, 3, 4]
    seeds = [ref.seed_points(tok[g, :cnt[g]], n, torch.float32) for g, n in enumerate(job.lens)]
    for side in (0, 1):
        got = job.chain(seeds, _layers_of(2, side), side, 0.5, K=K, cnt=cnt, scale=scale, h=h, w=w)
        pgot = job.chain([ref.seed_persons(n // 12, 12, side, torch.float32) for n in job.lens], _layers_of(2, side), side, 0.5, seg=12, scale=scale, h=h, w=w)
        for g, n in enumerate(job.lens):
            if n == 0:
                assert got[g].numel() == pgot[g].numel() == 0
                continue
            T = ref.rollout([job.full[l][g] for l in range(2)], 0.5)
            want = ref.rows_as_maps(ref.at_tokens(T, tok[g, :cnt[g]], side), h, w, scale)
            pwant = ref.as_maps(ref.reduce_persons(T, 12)[side], h, w, scale)
            e = max(_err(got[g].view(want.shape), want), _err(pgot[g].view(pwant.shape), pwant))
            print("x%d side %d group %d: max-abs %.2e" % (scale, side, g, e))
            assert e <= 2 * TOL


def test_raw_rejects_bad_arguments():
    L = cabi.lib()
    assert L.i2r_attn_rollout_step(None, None) == -1 and b"null pointer" in L.i2r_last_error()
    assert L.i2r_attn_rollout_step(ctypes.byref(cabi.AttnRolloutArgs()), None) == -1 and b"null pointer" in L.i2r_last_error()
    buf = torch.zeros(4096, device="cuda")
    out = torch.full((4096,), CANARY, device="cuda")
    rows = torch.full((4096,), CANARY, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int64, device="cuda")
    host_off = (ctypes.c_int32 * 3)(0, 10, 300)

    def args(**kw):
        d = dict(qk=buf.data_ptr(), in_=buf.data_ptr() + 1024, out=out.data_ptr(), grp_off=ibuf.data_ptr(), x_off=ibuf.data_ptr(), out_off=ibuf.data_ptr(),
                 ws=buf.data_ptr(), rows=rows.data_ptr(), grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=1, heads=1, hp=16, k_off=16, qk_cs=32,
                 ws_stride=2, K=3, seg=0, side=0, scale=1, h=1, w=1, alpha=0.5)
        d.update(kw)
        return cabi.AttnRolloutArgs(**d)

    for ptr in ("qk", "in_", "out", "grp_off", "x_off", "ws", "grp_off_host"):
        assert L.i2r_attn_rollout_step(ctypes.byref(args(**{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    nan = float("nan")
    for kw, msg in ((dict(in_=out.data_ptr()), b"in == out"), (dict(side=2), b"side=2"), (dict(side=-1), b"side=-1"), (dict(alpha=-0.1), b"alpha="),
                    (dict(alpha=1.5), b"alpha="), (dict(alpha=nan), b"alpha="), (dict(scale=0), b"scale=0"), (dict(scale=65), b"scale=65"),
                    (dict(seg=-2), b"seg=-2"), (dict(K=0), b"K=0"), (dict(K=1 << 20), b"K="), (dict(seg=3), b"not a multiple"), (dict(seg=4), b"not a multiple"),
                    (dict(scale=2, h=2, w=2), b"not a multiple"), (dict(scale=2, h=0, w=5), b"h=0"), (dict(scale=2, h=5, w=2, rows=None), b"scale > 1 needs"),
                    (dict(scale=2, h=5, w=2, out_off=None), b"scale > 1 needs"), (dict(scale=2, h=5, w=2, rows=buf.data_ptr() + 1024), b"scale > 1 needs"),
                    (dict(heads=0), b"heads=0"), (dict(hp=24, k_off=24, qk_cs=48), b"hp=24"), (dict(hp=272, k_off=272, qk_cs=544), b"hp=272"),
                    (dict(k_off=8), b"row stride"), (dict(k_off=18, qk_cs=36), b"row stride"), (dict(qk_cs=28), b"row stride"), (dict(qk_cs=34), b"row stride"),
                    (dict(qk=buf.data_ptr() + 4), b"alignment"), (dict(ws=buf.data_ptr() + 4), b"alignment"),
                    (dict(ws_stride=3), b"ws_stride=3"), (dict(ws_stride=0), b"ws_stride=0"), (dict(heads=2, k_off=32, qk_cs=64), b"ws_stride=2"),
                    (dict(n_grp=2, ws_stride=4), b"ws_stride=4"),  # the second group has 290 tokens: three key blocks
                    (dict(n_grp=0), b"n_grp=0"), (dict(n_grp=65536), b"n_grp=65536")):
        assert L.i2r_attn_rollout_step(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    torch.cuda.synchronize()
    assert not buf.any() and (out == CANARY).all() and (rows == CANARY).all(), "a rejected call launched something"


# ---------------------------------------------------------------------------------------------------------------------------------
# through rollout_at / person_rollout
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL_TAGS = ["w48_l31", "tph_l21", "hrt_l21", "w48_nh8_l21"]


def _net(cfg, sd, precision="fp32"):
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    if precision != "fp32":
        net.set_precision(precision)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _restated(tag, length=None):
    """(cfg, sd, x, m, length, restated maps, stack inputs): computed once per (tag, grouping), never modified"""
    cfg, sd, x, m, own, _ = setup(tag)
    length = list(length) if length is not None else own
    assert sum(length) == sum(own)
    maps, feats, _ = restate(cfg, sd, x, m, length)
    return cfg, sd, x, m, length, maps, feats


def _hook_maps(net, st, n_layers, x, m, length, lens):
    """one hooked forward: -> (output, per layer, per batch entry of the stack the [L, L] map its self_attn hook got)"""
    rec = {}
    layers = dict(net.named_modules())[st + ".layers"]
    hooks = [layers[i].self_attn.register_forward_hook(lambda mod, inp, out, i=i: rec.__setitem__(i, out[1])) for i in range(n_layers)]
    y = net(x, m, length)
    for hk in hooks:
        hk.remove()
    return y, [[rec[i][b, :n, :n] for b, n in enumerate(lens)] for i in range(n_layers)]


def _points(S, K, H, W, seed):
    import numpy as np
    rng = np.random.RandomState(seed)
    pts = torch.from_numpy(np.stack([rng.uniform(0, W, size=(S, K)), rng.uniform(0, H, size=(S, K))], -1))
    pts[0, 1] = float("nan")
    return pts


def _tables(st, pts, length, H, W, fh, fw):
    """per batch entry of the stack: (its query tokens, its token count), as rollout_at lays the points out"""
    from i2r_amd.models._base import group_tokens, points_to_tokens
    tok = points_to_tokens(pts, H, W, fh, fw)
    if st.startswith("singleformer."):
        return list(tok), [fh * fw] * sum(length)
    table, counts = group_tokens(tok, length, fh * fw)
    return [table[b, :c] for b, c in enumerate(counts)], [n * fh * fw for n in length]


def _check_points(got, per_layer, tabs, lens, side, alpha, fh, fw, scale, tol, what):
    """got: one stack's maps of rollout_at; per_layer[l][b]: the [L, L] maps of the rolled-out layers, lo .. hi -> worst max-abs; the rows of
    a dependency result sum to 1 within steps x 1e-5"""
    worst = 0.0
    for b, n in enumerate(lens):
        T = ref.rollout([layer[b].cuda() for layer in per_layer], alpha)
        want = ref.rows_as_maps(ref.at_tokens(T, tabs[b], side), fh, fw, scale)
        assert tuple(got[b].shape) == tuple(want.shape), (got[b].shape, want.shape)
        e = _err(got[b], want)
        worst = max(worst, e)
        assert e <= tol, "entry %d side %d: max-abs %.2e vs %s" % (b, side, e, what)
        if side == 0 and scale == 1:
            live = [k for k, t in enumerate(tabs[b]) if int(t) >= 0]
            s = (got[b].double().reshape(len(tabs[b]), -1)[live].sum(1) - 1).abs().max().item()
            assert s <= len(per_layer) * TOL, "entry %d: rows sum to 1 +- %.2e" % (b, s)
    return worst


@pytest.mark.parametrize("tag", MODEL_TAGS)
def test_rollout_at_matches_the_float64_chain_of_the_restated_maps(tag):
    cfg, sd, x, m, length, maps, feats = _restated(tag)
    net = _net(cfg, sd)
    eng = net.engine()
    H, W = x.shape[2:]
    xd, md = x.cuda(), m.cuda()
    y0 = net(xd, md, length)
    y0 = (y0["multi"] if isinstance(y0, dict) else y0).clone()
    pts = _points(sum(length), 3, H, W, 11)
    stacks = eng.capture_stacks()
    for side, mode in enumerate(("dependency", "affect")):
        for up in (False, True):
            y, got = net.rollout_at(xd, md, length, pts, mode=mode, upsample=up)
            torch.cuda.synchronize()
            assert torch.equal(y["multi"] if isinstance(y, dict) else y, y0), "rollout_at's heat maps differ from the default forward's"
            assert set(got) == set(stacks)
            for st, n_layers in stacks.items():
                fh, fw = feats[st].shape[2:]
                tabs, lens = _tables(st, pts, length, H, W, fh, fw)
                per_layer = [[maps[(st, l)][b, :n, :n] for b, n in enumerate(lens)] for l in range(n_layers)]
                w = _check_points(got[st], per_layer, tabs, lens, side, 0.5, fh, fw, H // fh if up else 1, TOL_MODEL, "the restatement")
                print("%s %s %s x%d, %d layers: max-abs vs the float64 chain %.2e" % (tag, st, mode, H // fh if up else 1, n_layers, w))
    # a sub-range and another alpha; a single layer at alpha = 1 is attention_at's map of that layer
    for st, n_layers in stacks.items():
        fh, fw = feats[st].shape[2:]
        tabs, lens = _tables(st, pts, length, H, W, fh, fw)
        lo, hi = (1, n_layers - 1) if n_layers > 1 else (0, 0)
        _, got = net.rollout_at(xd, md, length, pts, mode="affect", stacks=[st], layers={st: (lo, hi)}, alpha=0.25, upsample=False)
        assert set(got) == {st}
        per_layer = [[maps[(st, l)][b, :n, :n] for b, n in enumerate(lens)] for l in range(lo, hi + 1)]
        _check_points(got[st], per_layer, tabs, lens, 1, 0.25, fh, fw, 1, TOL_MODEL, "the restatement (layers %d .. %d)" % (lo, hi))
        for mode in ("dependency", "affect"):
            _, one = net.rollout_at(xd, md, length, pts, mode=mode, stacks=st, layers=(hi, hi), alpha=1.0, upsample=False)
            _, at = net.attention_at(xd, md, length, pts, mode=mode, layers={(st, hi)}, upsample=False)
            e = max(_err(a, b.double()) for a, b in zip(one[st], at[(st, hi)]))
            print("%s %s %s: one layer at alpha 1 vs attention_at %.2e" % (tag, st, mode, e))
            assert e <= TOL
    with pytest.raises(ValueError):
        net.rollout_at(xd, md, length, pts, layers={(next(iter(stacks)), 0), (next(iter(stacks)), 2)})
    with pytest.raises(ValueError):
        net.rollout_at(xd, md, length, pts, flip_pairs=[[1, 2]])


@pytest.mark.parametrize("tag", MODEL_TAGS)
def test_person_rollout_matches_the_float64_chain_of_the_restated_maps(tag):
    cfg, sd, x, m, length, maps, feats = _restated(tag)
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    fh, fw = feats[st].shape[2:]
    hw, down = fh * fw, x.shape[2] // fh
    xd, md = x.cuda(), m.cuda()
    lens = [n * hw for n in length]
    red = [ref.reduce_persons(ref.rollout([maps[(st, l)][b, :n, :n].cuda() for l in range(n_layers)], 0.5), hw) for b, n in enumerate(lens)]
    for kind in (None, "dependency", "affect"):
        for up in ((False,) if kind is None else (False, True)):
            y, res = net.person_rollout(xd, md, length, maps=kind, upsample=up)
            torch.cuda.synchronize()
            assert set(res.relation) == {st} and set(res.maps) == ({st} if kind else set())
            for b, n in enumerate(length):
                D, F, R, _ = red[b]
                assert res.relation[st][b].shape == (n, n)
                errs = [_err(res.relation[st][b], R), (res.relation[st][b].double().sum(1) - 1).abs().max().item()]
                if kind:
                    want = ref.as_maps(D if kind == "dependency" else F, fh, fw, down if up else 1)
                    assert res.maps[st][b].shape == want.shape
                    errs.append(_err(res.maps[st][b], want))
                    if not up:
                        rows = res.maps[st][b].double().reshape(n, n * hw)
                        sums = (rows.sum(1) - 1).abs().max().item() if kind == "dependency" else (rows.sum(0) - 1).abs().max().item()
                        assert sums <= n_layers * TOL, "%s image %d maps=%s: sums to 1 +- %.2e" % (tag, b, kind, sums)
                print("%s image %d maps=%s x%d: max-abs vs the float64 chain %.2e" % (tag, b, kind, down if up else 1, max(errs)))
                assert max(errs) <= TOL_MODEL
    hi = n_layers - 1
    for kind in ("dependency", "affect"):
        _, one = net.person_rollout(xd, md, length, maps=kind, layers=(hi, hi), alpha=1.0)
        _, rel = net.person_relations(xd, md, length, maps=kind, layers={(st, hi)})
        e = max(max(_err(a, b.double()) for a, b in zip(one.relation[st], rel.relation[(st, hi)])),
                max(_err(a, b.double()) for a, b in zip(one.maps[st], rel.maps[(st, hi)])))
        print("%s maps=%s: one layer at alpha 1 vs person_relations %.2e" % (tag, kind, e))
        assert e <= TOL
    with pytest.raises(ValueError):
        net.person_rollout(xd, md, length, layers={("singleformer.global_encoder", 0), (st, 0)})
    with pytest.raises(ValueError):
        net.person_rollout(xd, md, length, flip_pairs=[[1, 2]])
    with pytest.raises(ValueError):
        eng.forward_groups(xd, md, torch.zeros(1, dtype=torch.int32), [1], rollout=object())


def test_bf16_results_are_the_float64_chain_of_the_same_models_hook_maps():
    cfg, sd, x, m, length, _ = setup("tph_l21")
    net = _net(cfg, sd, "bf16")
    eng = net.engine()
    H, W = x.shape[2:]
    xd, md = x.cuda(), m.cuda()
    pts = _points(sum(length), 3, H, W, 5)
    sizes = eng.capture_map_sizes(H, W)
    for st, n_layers in eng.capture_stacks().items():
        fh, fw = sizes[st]
        tabs, lens = _tables(st, pts, length, H, W, fh, fw)
        yh, hooked = _hook_maps(net, st, n_layers, xd, md, length, lens)
        for side, mode in enumerate(("dependency", "affect")):
            y, got = net.rollout_at(xd, md, length, pts, mode=mode, stacks=[st], upsample=False)
            torch.cuda.synchronize()
            assert torch.equal(y["multi"] if isinstance(y, dict) else y, yh["multi"] if isinstance(yh, dict) else yh)
            w = _check_points(got[st], hooked, tabs, lens, side, 0.5, fh, fw, 1, n_layers * TOL, "the bf16 model's hook maps")
            print("tph_l21 bf16 %s %s: max-abs vs the chain of the hooks' maps %.2e (bar %d x 1e-5)" % (st, mode, w, n_layers))
        if st == eng.inter_stack:
            for kind in ("dependency", "affect"):
                _, res = net.person_rollout(xd, md, length, maps=kind)
                for b, n in enumerate(length):
                    D, F, R, _ = ref.reduce_persons(ref.rollout([layer[b] for layer in hooked], 0.5), fh * fw)
                    e = max(_err(res.relation[st][b], R), _err(res.maps[st][b], ref.as_maps(D if kind == "dependency" else F, fh, fw)))
                    print("tph_l21 bf16 image %d maps=%s: max-abs vs the chain of the hooks' maps %.2e" % (b, kind, e))
                    assert e <= n_layers * TOL


def test_regroup_at_the_same_capacity_builds_nothing_and_the_default_program_is_untouched():
    cfg, sd, x, m, length, maps, feats = _restated("w48_l31")
    assert length == [3, 1]
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    fh, fw = feats[st].shape[2:]
    H, W = x.shape[2:]
    xd, md = x.cuda(), m.cuda()
    y0 = net(xd, md, length).clone()
    (key0, entry0), = eng.programs.items()
    ops0 = [(k, lane) for k, lane, _ in entry0[0].ops]
    builds = None
    for i, ln in enumerate(([3, 1], [2, 2], [1, 3], [3, 1])):
        mp = maps if ln == [3, 1] else _restated("w48_l31", tuple(ln))[5]
        pts = _points(sum(ln), 3, H, W, 20 + i)  # (new points every call)
        _, got = net.rollout_at(xd, md, ln, pts, stacks=[st], upsample=False, alpha=0.5 + 0.1 * i)
        _, res = net.person_rollout(xd, md, ln, maps="affect", upsample=2)
        torch.cuda.synchronize()
        if i == 0:
            builds = eng.n_builds
        assert eng.n_builds == builds, "a regroup at the same capacity rebuilt a program"
        tabs, lens = _tables(st, pts, ln, H, W, fh, fw)
        per_layer = [[mp[(st, l)][b, :n, :n] for b, n in enumerate(lens)] for l in range(n_layers)]
        _check_points(got[st], per_layer, tabs, lens, 0, 0.5 + 0.1 * i, fh, fw, 1, TOL_MODEL, "the restatement")
        for b, n in enumerate(lens):
            F = ref.reduce_persons(ref.rollout([layer[b].cuda() for layer in per_layer], 0.5), fh * fw)[1]
            assert _err(res.maps[st][b], ref.as_maps(F, fh, fw, 2)) <= TOL_MODEL
    assert len(eng.programs) == 3 and eng.programs[key0] is entry0
    assert [(k, lane) for k, lane, _ in eng.programs[key0][0].ops] == ops0, "the default program's op list changed"
    assert torch.equal(net(xd, md, length), y0) and eng.n_builds == builds, "a plain forward afterwards differs"
