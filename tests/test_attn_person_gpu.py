"""-m gpu: the attention per person on the MI355X -- the raw i2r_attn_person_maps C-ABI (relation matrices, dependency and affect maps,
up-sampling, bad arguments) against the float64 reference (tests/_attn_person_ref.py) and against what i2r_attn_weights writes, and
net.person_relations against the CPU restatement (tests/_attn_ref.py), the maps the forward hooks get and net.attention_at.
Every test prints the figures it asserts on (pytest -s).  Measured on the MI355X (max-abs): raw against float64 R 1.4e-7, D 1.4e-7,
F 5.3e-7, sum identities 3.9e-7, against the full capture's block sums 3.2e-7, up-sampled D 3.3e-9 / F 4.9e-7 -- all under the 1e-5 bar,
which therefore stays; through the model against the restatement 1.5e-5 (bar 1e-3), against the hooks' maps 6.2e-7 (bar 1e-5)."""
import ctypes
import functools

import pytest
import torch

from _attn_person_ref import as_maps, full_map, reduce_persons
from _attn_query_ref import point_of_token
from _attn_ref import restate
from _golden import setup
from i2r_amd import cabi, models

pytestmark = pytest.mark.gpu
TOL = 1e-5       # the bar the full maps and their row sums meet against float64 (tests/test_attn_maps_gpu.py): every output is a partial
                 # row sum or an average of those entries
TOL_MODEL = 1e-3  # the bar of the hook tests against the CPU restatement
CANARY = 12345.0
# (tokens per person T, persons of every group of the launch, first group offset): an empty group inside, offsets that are no multiples
# of 4, and behind each launch's groups one more group that n_grp excludes
CASES = [
    (12, [1, 0, 2], 3),    # R = [[1]]; a person boundary inside a 16-key tile
    (20, [5, 0, 1], 1),    # five persons, T no multiple of 16
    (192, [3], 0),         # boundaries inside 128-key blocks, L = 576
    (432, [2], 2),         # the 384 x 288 token count: 27 key tiles per person
    (1, [4, 0, 3], 5),     # one token per person
]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
# raw C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _make_qk(heads, hp, n_tok, seed):
    """q|k rows as tests/test_attn_maps_gpu.py draws them: pad dims exactly 0, k behind a gap, a row stride with a tail"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    hd = hp - 3 if hp > 16 else hp
    hs = heads * hp
    k_off = hs + 16
    qk_cs = k_off + hs + 8
    qk = torch.zeros(n_tok, qk_cs, device="cuda")
    for h in range(heads):
        qk[:, h * hp:h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g) * 2.0 * hd ** -0.5
        qk[:, k_off + h * hp:k_off + h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g)
    return qk, k_off, qk_cs


class _Launch:
    """the tables of one case: groups of pers[g] * T tokens from token `start`, then one group of 2 T tokens outside n_grp"""

    def __init__(self, T, pers, start, heads, hp, seed):
        self.T, self.pers, self.heads, self.hp = T, pers, heads, hp
        self.n_grp = len(pers)
        self.offs = [start]
        for p in list(pers) + [2]:
            self.offs.append(self.offs[-1] + p * T)
        self.lens = [p * T for p in pers]
        self.qk, self.k_off, self.qk_cs = _make_qk(heads, hp, self.offs[-1], seed)
        self.goff = torch.tensor(self.offs, dtype=torch.int32, device="cuda")
        self.host_off = (ctypes.c_int32 * (self.n_grp + 1))(*self.offs[:self.n_grp + 1])
        self.stride = 2 * heads * max(-(-n // 128) for n in self.lens)

    @functools.cached_property
    def full(self):
        """float64 [L, L] maps of the computed groups (None for an empty one)"""
        return [full_map(self.qk[o:o + n], self.heads, self.hp, self.k_off) if n else None for o, n in zip(self.offs, self.lens)]

    def run(self, mode, scale=1, h=1, w=1, first=7, gap=5):
        """one i2r_attn_person_maps call into blocks separated by canary gaps -> (rel blocks, maps blocks or None), canaries checked"""
        r_off, m_off, rpos, mpos = [], [], 3, first
        for p, n in zip(self.pers, self.lens):
            r_off.append(rpos)
            m_off.append(mpos)
            rpos += p * p + gap
            mpos += (p * n * scale * scale if mode else 0) + gap
        rel = torch.full((rpos + 16,), CANARY, device="cuda")
        maps = torch.full((mpos + 64,), CANARY, device="cuda")
        n_tok = self.offs[self.n_grp]
        need = (2 if mode == 1 and scale > 1 else 1) * max(self.pers) * n_tok
        rows = torch.full((need + 8,), CANARY, device="cuda")
        ws = torch.empty(self.stride * n_tok, device="cuda")
        d_roff = torch.tensor(r_off, dtype=torch.int64, device="cuda")
        d_moff = torch.tensor(m_off, dtype=torch.int64, device="cuda")
        a = cabi.AttnPersonArgs(qk=self.qk.data_ptr(), grp_off=self.goff.data_ptr(), ws=ws.data_ptr(), rel=rel.data_ptr(), rel_off=d_roff.data_ptr(),
                                maps=maps.data_ptr() if mode else None, maps_off=d_moff.data_ptr() if mode else None, rows=rows.data_ptr(),
                                grp_off_host=ctypes.cast(self.host_off, ctypes.c_void_p), n_grp=self.n_grp, heads=self.heads, hp=self.hp,
                                k_off=self.k_off, qk_cs=self.qk_cs, ws_stride=self.stride, seg=self.T, mode=mode, scale=scale, h=h, w=w)
        cabi.check(cabi.lib().i2r_attn_person_maps(ctypes.byref(a), _stream()), "i2r_attn_person_maps")
        torch.cuda.synchronize()
        assert (rows[need:] == CANARY).all(), "a store behind the rows workspace"
        written = torch.zeros(rel.numel(), dtype=torch.bool, device="cuda")
        for o, p in zip(r_off, self.pers):
            written[o:o + p * p] = True
        assert (rel[~written] == CANARY).all(), "a store outside the computed relation blocks"
        assert not (rel[written] == CANARY).any(), "a relation entry was not written"
        R = [rel[o:o + p * p].view(p, p) for o, p in zip(r_off, self.pers)]
        if not mode:
            assert (maps == CANARY).all(), "mode 0 wrote maps"
            return R, None
        written = torch.zeros(maps.numel(), dtype=torch.bool, device="cuda")
        sizes = [p * n * scale * scale for p, n in zip(self.pers, self.lens)]
        for o, n in zip(m_off, sizes):
            written[o:o + n] = True
        assert (maps[~written] == CANARY).all(), "a store outside the computed map blocks"
        assert not (maps[written] == CANARY).any(), "a map entry was not written"
        return R, [maps[o:o + n] for o, n in zip(m_off, sizes)]

    def full_capture(self):
        """what i2r_attn_weights writes for the same rows: per computed group the fp32 [L, L] map"""
        o_off, pos = [], 0
        for n in self.lens:
            o_off.append(pos)
            pos += n * n
        out = torch.zeros(max(pos, 1), device="cuda")
        ws = torch.empty(self.stride * self.offs[self.n_grp], device="cuda")
        ooff = torch.tensor(o_off, dtype=torch.int64, device="cuda")
        tiles = sum(-(-n // 16) * -(-n // 128) for n in self.lens)
        a = cabi.AttnWeightsArgs(self.qk.data_ptr(), out.data_ptr(), self.goff.data_ptr(), ooff.data_ptr(), ws.data_ptr(), self.n_grp, self.heads, self.hp,
                                 self.k_off, self.qk_cs, tiles, self.stride)
        cabi.check(cabi.lib().i2r_attn_weights(ctypes.byref(a), _stream()), "i2r_attn_weights")
        torch.cuda.synchronize()
        return [out[o:o + n * n].view(n, n) for o, n in zip(o_off, self.lens)]


def _err(got, ref):
    return (got.double() - ref).abs().max().item() if ref.numel() else 0.0


@pytest.mark.parametrize("heads,hp", [(1, 96), (1, 80), (2, 48), (8, 16)])
def test_raw_relation_dependency_and_affect_match_float64(heads, hp):
    worst = dict(R=0.0, D=0.0, F=0.0, sums=0.0, capture=0.0)
    for ci, (T, pers, start) in enumerate(CASES):
        job = _Launch(T, pers, start, heads, hp, 1000 * heads + hp + ci)
        ref = [reduce_persons(f, T) if f is not None else None for f in job.full]
        cap = [reduce_persons(f, T) if f.numel() else None for f in job.full_capture()]  # float64 block sums of the fp32 full maps
        R0, _ = job.run(0)
        R1, Dm = job.run(1, first=8)   # (a first block at a multiple of 4 as well)
        R2, Fm = job.run(2)
        R2b, Fb = job.run(2)
        for g, p in enumerate(pers):
            if p == 0:
                assert Dm[g].numel() == Fm[g].numel() == R0[g].numel() == 0
                continue
            n = p * T
            D, F, R, _ = ref[g]
            got_d, got_f = Dm[g].view(p, n), Fm[g].view(p, n)
            assert torch.equal(R0[g], R1[g]) and torch.equal(R0[g], R2[g]), "R differs between the modes"
            assert torch.equal(R2[g], R2b[g]) and torch.equal(Fm[g], Fb[g]), "two runs differ"
            worst["R"], worst["D"], worst["F"] = max(worst["R"], _err(R0[g], R)), max(worst["D"], _err(got_d, D)), max(worst["F"], _err(got_f, F))
            sums = max((R0[g].double().sum(1) - 1).abs().max().item(), (got_d.double().sum(1) - 1).abs().max().item(),
                       (got_f.double().sum(0) - 1).abs().max().item())
            worst["sums"] = max(worst["sums"], sums)
            worst["capture"] = max(worst["capture"], _err(got_d, cap[g][0]), _err(got_f, cap[g][1]))
            if p == 1:
                assert abs(R0[g].item() - 1) <= TOL
    print("heads=%d hp=%d: max-abs vs float64 R %.2e D %.2e F %.2e, sum identities %.2e, vs the full capture's block sums %.2e"
          % (heads, hp, worst["R"], worst["D"], worst["F"], worst["sums"], worst["capture"]))
    for name, e in worst.items():
        assert e <= TOL, "heads=%d hp=%d: %s max-abs %.2e" % (heads, hp, name, e)


@pytest.mark.parametrize("scale", [2, 4])
def test_raw_upsampling_matches_float64_interpolate(scale):
    T, h, w = 192, 16, 12
    for heads, hp in ((2, 48), (1, 80)):
        job = _Launch(T, [3, 0, 1], 0, heads, hp, 77 + scale + hp)
        ref = [reduce_persons(f, T) if f is not None else None for f in job.full]
        R0, _ = job.run(0, scale=scale, h=h, w=w)
        for mode in (1, 2):
            R, M = job.run(mode, scale=scale, h=h, w=w, first=7 if mode == 1 else 4)
            for g, p in enumerate(job.pers):
                if p == 0:
                    continue
                want = as_maps(ref[g][mode - 1], h, w, scale)
                assert M[g].numel() == want.numel() == p * p * T * scale * scale
                err = _err(M[g].view(want.shape), want)
                print("x%d heads=%d mode %d group %d: max-abs %.2e" % (scale, heads, mode, g, err))
                assert err <= TOL, "x%d heads=%d mode %d group %d: max-abs %.2e" % (scale, heads, mode, g, err)
                assert torch.equal(R[g], R0[g])


def test_raw_rejects_bad_arguments():
    L = cabi.lib()
    assert L.i2r_attn_person_maps(None, None) == -1 and b"null pointer" in L.i2r_last_error()
    assert L.i2r_attn_person_maps(ctypes.byref(cabi.AttnPersonArgs()), None) == -1 and b"null pointer" in L.i2r_last_error()
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int64, device="cuda")
    host_off = (ctypes.c_int32 * 3)(0, 10, 300)

    def args(**kw):
        d = dict(qk=buf.data_ptr(), grp_off=ibuf.data_ptr(), ws=buf.data_ptr(), rel=buf.data_ptr(), rel_off=ibuf.data_ptr(), maps=buf.data_ptr(),
                 maps_off=ibuf.data_ptr(), rows=buf.data_ptr(), grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=1, heads=1, hp=16,
                 k_off=16, qk_cs=32, ws_stride=2, seg=5, mode=1, scale=1, h=1, w=1)
        d.update(kw)
        return cabi.AttnPersonArgs(**d)

    for ptr in ("qk", "grp_off", "ws", "rel", "rel_off", "rows", "grp_off_host", "maps", "maps_off"):
        assert L.i2r_attn_person_maps(ctypes.byref(args(**{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    for kw, msg in ((dict(mode=3), b"mode=3"), (dict(mode=-1), b"mode=-1"), (dict(scale=0), b"scale=0"), (dict(scale=65), b"scale=65"),
                    (dict(seg=0), b"seg=0"), (dict(seg=-2), b"seg=-2"), (dict(seg=3), b"not a multiple of seg"), (dict(seg=4), b"not a multiple of seg"),
                    (dict(scale=2, h=2, w=2), b"is not h w"), (dict(scale=2, h=0, w=5), b"is not h w"), (dict(scale=2, h=5, w=1, mode=0, seg=10), b"is not h w"),
                    (dict(heads=0), b"heads=0"), (dict(hp=24, k_off=24, qk_cs=48), b"hp=24"), (dict(hp=272, k_off=272, qk_cs=544), b"hp=272"),
                    (dict(k_off=8), b"row stride"), (dict(k_off=18, qk_cs=36), b"row stride"), (dict(qk_cs=28), b"row stride"), (dict(qk_cs=34), b"row stride"),
                    (dict(qk=buf.data_ptr() + 4), b"alignment"), (dict(ws=buf.data_ptr() + 4), b"alignment"),
                    (dict(ws_stride=3), b"ws_stride=3"), (dict(ws_stride=0), b"ws_stride=0"), (dict(heads=2, k_off=32, qk_cs=64), b"ws_stride=2"),
                    (dict(n_grp=2, ws_stride=4), b"ws_stride=4"),  # the second group has 290 tokens: three key blocks
                    (dict(n_grp=0), b"n_grp=0"), (dict(n_grp=65536), b"n_grp=65536")):
        assert L.i2r_attn_person_maps(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    torch.cuda.synchronize()
    assert not buf.any(), "a rejected call launched something"


# ---------------------------------------------------------------------------------------------------------------------------------
# through person_relations
# ---------------------------------------------------------------------------------------------------------------------------------
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


def _hook_maps(net, st, n_layers, x, m, length, hw):
    """one hooked forward: -> (heat maps, {layer: per image the [L, L] map its self_attn hook got})"""
    rec = {}
    layers = dict(net.named_modules())[st + ".layers"]
    hooks = [layers[i].self_attn.register_forward_hook(lambda mod, inp, out, i=i: rec.__setitem__(i, out[1])) for i in range(n_layers)]
    y = net(x, m, length)
    for hk in hooks:
        hk.remove()
    return y, {i: [w[b, :n * hw, :n * hw] for b, n in enumerate(length)] for i, w in rec.items()}


def _check_against(res, kind, scale, st, per_layer, length, fh, fw, tol, what):
    """res of person_relations(maps=kind, scale) against the reduction of per_layer[l][b] = [L, L] maps -> worst max-abs"""
    worst = 0.0
    assert set(res.relation) == {(st, l) for l in per_layer} and set(res.maps) == (set(res.relation) if kind else set())
    for l, full in per_layer.items():
        for b, n in enumerate(length):
            D, F, R, _ = reduce_persons(full[b], fh * fw)
            assert res.relation[(st, l)][b].shape == (n, n)
            errs = [_err(res.relation[(st, l)][b], R.to(res.relation[(st, l)][b].device))]
            if kind:
                want = as_maps(D if kind == "dependency" else F, fh, fw, scale)
                got = res.maps[(st, l)][b]
                assert got.shape == (n, n, fh * scale, fw * scale), got.shape
                errs.append(_err(got, want.to(got.device)))
            worst = max(worst, *errs)
            assert max(errs) <= tol, "%s layer %d image %d maps=%s x%d: max-abs %.2e vs %s" % (st, l, b, kind, scale, max(errs), what)
    return worst


@pytest.mark.parametrize("tag", ["w48_l31", "tph_l21", "hrt_l21"])
def test_person_relations_match_restatement_hooks_and_attention_at(tag):
    cfg, sd, x, m, length, maps, feats = _restated(tag)
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    fh, fw = feats[st].shape[2:]
    hw, down = fh * fw, x.shape[2] // fh
    xd, md = x.cuda(), m.cuda()
    y0 = net(xd, md, length)
    y0 = (y0["multi"] if isinstance(y0, dict) else y0).clone()
    yh, hooked = _hook_maps(net, st, n_layers, xd, md, length, hw)
    restated = {l: [maps[(st, l)][b, :n * hw, :n * hw] for b, n in enumerate(length)] for l in range(n_layers)}
    for kind in (None, "dependency", "affect"):
        for up in ((False,) if kind is None else (False, True)):
            y, res = net.person_relations(xd, md, length, maps=kind, upsample=up)
            torch.cuda.synchronize()
            assert torch.equal(y["multi"] if isinstance(y, dict) else y, y0), "person_relations' heat maps differ from the default forward's"
            scale = down if up else 1
            w1 = _check_against(res, kind, scale, st, restated, length, fh, fw, TOL_MODEL, "the restatement")
            w2 = _check_against(res, kind, scale, st, hooked, length, fh, fw, TOL, "the hooks' maps")
            print("%s %s maps=%s x%d: max-abs vs restatement %.2e, vs the hooks' maps %.2e" % (tag, st, kind, scale, w1, w2))
            for l in range(n_layers):  # every image's tensors are views of one buffer
                assert all(v.untyped_storage().data_ptr() == res.relation[(st, 0)][0].untyped_storage().data_ptr()
                           for v in res.relation[(st, l)] + (res.maps[(st, l)] if kind else []))
    # dependency maps = the mean over a person's T query tokens of attention_at's dependency rows at every token centre of the crop
    pts = torch.tensor([[point_of_token(t, fw, down) for t in range(hw)]] * sum(length), dtype=torch.float64)
    _, at = net.attention_at(xd, md, length, pts, mode="dependency", upsample=False, layers={(st, l) for l in range(n_layers)})
    _, res = net.person_relations(xd, md, length, maps="dependency")
    for l in range(n_layers):
        for b, n in enumerate(length):
            mean = at[(st, l)][b].view(n, hw, n, fh, fw).double().mean(1)
            err = _err(res.maps[(st, l)][b], mean)
            assert err <= TOL, "%s layer %d image %d: dependency maps vs the mean of attention_at's rows: max-abs %.2e" % (tag, l, b, err)
    with pytest.raises(ValueError):
        net.person_relations(xd, md, length, layers={("singleformer.global_encoder", 0), (st, 0)})
    with pytest.raises(ValueError):
        eng.forward_groups(xd, md, torch.zeros(1, dtype=torch.int32), [1], persons=object())


def test_regroup_at_the_same_capacity_builds_nothing_and_default_program_is_untouched():
    cfg, sd, x, m, length, maps, feats = _restated("w48_l31")
    assert length == [3, 1]
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    fh, fw = feats[st].shape[2:]
    xd, md = x.cuda(), m.cuda()
    y0 = net(xd, md, length).clone()
    (key0, entry0), = eng.programs.items()
    ops0 = [(k, lane) for k, lane, _ in entry0[0].ops]
    builds = prog = None
    for i, (ln, mp) in enumerate((([3, 1], maps), ([2, 2], None), ([1, 3], None), ([3, 1], maps))):
        if mp is None:
            mp = _restated("w48_l31", tuple(ln))[5]
        _, res = net.person_relations(xd, md, ln, maps="affect", upsample=2)
        torch.cuda.synchronize()
        key, = [k for k in eng.programs if "persons" in k]
        if i == 0:
            builds, prog = eng.n_builds, eng.programs[key][0]
        assert eng.n_builds == builds and eng.programs[key][0] is prog, "a regroup at the same capacity rebuilt the program"
        restated = {l: [mp[(st, l)][b, :n * fh * fw, :n * fh * fw] for b, n in enumerate(ln)] for l in range(n_layers)}
        _check_against(res, "affect", 2, st, restated, ln, fh, fw, TOL_MODEL, "the restatement")
    assert set(eng.programs) == {key0, key} and eng.programs[key0] is entry0
    assert [(k, lane) for k, lane, _ in eng.programs[key0][0].ops] == ops0, "the default program's op list changed"
    assert cabi.CAPTURE_OP_ATTN_PERSON not in [k for k, _ in ops0] and cabi.CAPTURE_OP_ATTN_PERSON in [k for k, _, _ in prog.ops]
    builds = eng.n_builds
    assert torch.equal(net(xd, md, length), y0) and eng.n_builds == builds


def test_bf16_outputs_are_the_reduction_of_the_same_models_hook_maps():
    cfg, sd, x, m, length, _ = setup("tph_l21")
    net = _net(cfg, sd, "bf16")
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    fh, fw = eng.capture_map_sizes(x.shape[2], x.shape[3])[st]
    xd, md = x.cuda(), m.cuda()
    yh, hooked = _hook_maps(net, st, n_layers, xd, md, length, fh * fw)
    for kind in ("dependency", "affect"):
        y, res = net.person_relations(xd, md, length, maps=kind)
        torch.cuda.synchronize()
        assert torch.equal(y["multi"] if isinstance(y, dict) else y, yh["multi"] if isinstance(yh, dict) else yh)
        worst = _check_against(res, kind, 1, st, hooked, length, fh, fw, TOL, "the bf16 model's hook maps")
        print("tph_l21 bf16 maps=%s: max-abs vs the hooks' maps %.2e" % (kind, worst))
