"""-m gpu: the target form of the attention per person on the MI355X -- the raw i2r_attn_target_maps C-ABI (r, D_t, F_t, up-sampling,
canaries, bad arguments) against the float64 reference (tests/_attn_person_ref.py, row 0) and bit for bit against row 0 of
i2r_attn_person_maps, and net.main_target_relations against net.forward_main_target and net.person_relations on the expanded batch.
Every test prints the figures it asserts on (pytest -s).  Measured on the MI355X (max-abs): raw against float64 r 1.2e-7, D_t 1.2e-7,
F_t 7.0e-7, sum identities 3.9e-7, up-sampled 4.1e-7 -- all under the 1e-5 bar; scale 1 bit-identical to row 0 of the person form in
every case; through the model against person_relations on the expanded batch 0.0 on all three paths (bars 1e-5 / 1e-3), image_relation
against the whole image's person_relations 3.0e-8; bf16 sum identities 2.4e-7."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from _attn_person_ref import full_map, reduce_persons
from _golden import setup
from i2r_amd import cabi, input as i2r_input, models

pytestmark = pytest.mark.gpu
TOL = 1e-5        # the raw bar of the attention-map kernels against float64 (tests/test_attn_person_gpu.py)
TOL_MODEL = 1e-3  # the model-level bar of these maps
NAN = float("nan")
MEMBERS = [1, 2, 3, 6]              # the groups of one call
SEGS = [1, 5, 12, 48, 192]          # tokens per member: ends inside a tile (1, 5, 12), L_g = 144 / 576 / 1152 (48 x 3, 192 x 3, 192 x 6)
HEADS = [(1, 96), (1, 80), (2, 48), (8, 16)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _make_qk(heads, hp, n_tok, seed):
    """q|k rows as tests/test_attn_person_gpu.py draws them: pad dims exactly 0, k behind a gap, a row stride with a tail"""
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


def _only(buf, spans, what):
    """buf was NaN everywhere: exactly the spans [(start, count)] are written now"""
    written = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    for o, n in spans:
        written[o:o + n] = True
    assert torch.isnan(buf[~written]).all(), "a store outside the computed %s blocks" % what
    assert not torch.isnan(buf[written]).any(), "an entry of a computed %s block was not written" % what


class _Launch:
    """the tables of one call: groups of pers[g] * seg tokens from token `start` (0 members: an empty group), all of them in the table;
    a call computes the first n_grp"""

    def __init__(self, seg, pers, start, heads, hp, seed):
        self.seg, self.pers, self.heads, self.hp = seg, list(pers), heads, hp
        self.offs = [start]
        for p in self.pers:
            self.offs.append(self.offs[-1] + p * seg)
        self.lens = [p * seg for p in self.pers]
        self.qk, self.k_off, self.qk_cs = _make_qk(heads, hp, self.offs[-1], seed)
        self.goff = torch.tensor(self.offs, dtype=torch.int32, device="cuda")
        self.stride = 2 * heads * max(-(-n // 128) for n in self.lens)

    @functools.cached_property
    def ref(self):
        """float64 (D, F, R) of every group (None for an empty one)"""
        return [reduce_persons(full_map(self.qk[o:o + n], self.heads, self.hp, self.k_off), self.seg)[:3] if n else None
                for o, n in zip(self.offs, self.lens)]

    def _tables(self, n_grp, rel_sizes, map_sizes, first, gap):
        r_off, m_off, rpos, mpos = [], [], 3, first
        for rs, ms in zip(rel_sizes, map_sizes):
            r_off.append(rpos)
            m_off.append(mpos)
            rpos += rs + gap
            mpos += ms + gap
        rel = torch.full((rpos + 16,), NAN, device="cuda")
        maps = torch.full((mpos + 64,), NAN, device="cuda")
        host_off = (ctypes.c_int32 * (n_grp + 1))(*self.offs[:n_grp + 1])
        return r_off, m_off, rel, maps, host_off

    def target(self, mode, scale=1, h=1, w=1, n_grp=None, first=7, gap=5):
        """one i2r_attn_target_maps call on NaN-filled, over-allocated buffers -> (r per group, maps blocks or None); what was written
        where is checked here: rel, maps, the rows workspace and the statistics workspace"""
        n_grp = len(self.pers) if n_grp is None else n_grp
        pers, lens, seg = self.pers[:n_grp], self.lens[:n_grp], self.seg
        msz = [n * scale * scale if mode else 0 for n in lens]
        r_off, m_off, rel, maps, host_off = self._tables(n_grp, pers, msz, first, gap)
        n_tok, total = self.offs[-1], self.offs[n_grp]
        rows = torch.full((2 * n_tok + 8,), NAN, device="cuda")
        ws = torch.full((self.stride * (n_tok + 4),), NAN, device="cuda")
        d_roff = torch.tensor(r_off, dtype=torch.int64, device="cuda")
        d_moff = torch.tensor(m_off, dtype=torch.int64, device="cuda")
        a = cabi.AttnTargetArgs(qk=self.qk.data_ptr(), grp_off=self.goff.data_ptr(), ws=ws.data_ptr(), rel=rel.data_ptr(), rel_off=d_roff.data_ptr(),
                                maps=maps.data_ptr() if mode else None, maps_off=d_moff.data_ptr() if mode else None, rows=rows.data_ptr(),
                                grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=n_grp, heads=self.heads, hp=self.hp,
                                k_off=self.k_off, qk_cs=self.qk_cs, ws_stride=self.stride, seg=seg, mode=mode, scale=scale, h=h, w=w)
        cabi.check(cabi.lib().i2r_attn_target_maps(ctypes.byref(a), _stream()), "i2r_attn_target_maps")
        torch.cuda.synchronize()
        _only(rel, list(zip(r_off, pers)), "relation")
        _only(maps, list(zip(m_off, msz)), "map")
        spans = []  # rows: F_t of group g at grp_off[g] (not for mode 2 at scale 1), the raw D_t (mode 1, scale > 1) grp_off[n_grp] behind
        if not (mode == 2 and scale == 1):
            spans += [(o, n) for o, n in zip(self.offs, lens)]
        if mode == 1 and scale > 1:
            spans += [(total + o, n) for o, n in zip(self.offs, lens)]
        _only(rows, spans, "rows workspace")
        wsr = ws.view(n_tok + 4, self.stride)
        target = torch.zeros(n_tok + 4, dtype=torch.bool, device="cuda")
        for o, n in zip(self.offs, lens):
            if n:
                target[o:o + seg] = True
                used = 2 * self.heads * -(-n // 128)
                assert not torch.isnan(wsr[o:o + seg, :used]).any() and torch.isnan(wsr[o:o + seg, used:]).all(), "the targets' statistics rows"
        assert torch.isnan(wsr[~target]).all(), "a statistics row of a token that is no target's was written"
        return [rel[o:o + p] for o, p in zip(r_off, pers)], ([maps[o:o + n] for o, n in zip(m_off, msz)] if mode else None)

    def person(self, mode):
        """i2r_attn_person_maps at scale 1 on the same rows -> (R per group, [P, L] blocks or None)"""
        n_grp = len(self.pers)
        msz = [p * n if mode else 0 for p, n in zip(self.pers, self.lens)]
        r_off, m_off, rel, maps, host_off = self._tables(n_grp, [p * p for p in self.pers], msz, 7, 5)
        n_tok = self.offs[-1]
        rows = torch.empty(max(self.pers) * n_tok + 8, device="cuda")
        ws = torch.empty(self.stride * n_tok, device="cuda")
        d_roff = torch.tensor(r_off, dtype=torch.int64, device="cuda")
        d_moff = torch.tensor(m_off, dtype=torch.int64, device="cuda")
        a = cabi.AttnPersonArgs(qk=self.qk.data_ptr(), grp_off=self.goff.data_ptr(), ws=ws.data_ptr(), rel=rel.data_ptr(), rel_off=d_roff.data_ptr(),
                                maps=maps.data_ptr() if mode else None, maps_off=d_moff.data_ptr() if mode else None, rows=rows.data_ptr(),
                                grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=n_grp, heads=self.heads, hp=self.hp,
                                k_off=self.k_off, qk_cs=self.qk_cs, ws_stride=self.stride, seg=self.seg, mode=mode, scale=1, h=1, w=1)
        cabi.check(cabi.lib().i2r_attn_person_maps(ctypes.byref(a), _stream()), "i2r_attn_person_maps")
        torch.cuda.synchronize()
        return ([rel[o:o + p * p].view(p, p) for o, p in zip(r_off, self.pers)],
                [maps[o:o + n].view(p, -1) for o, n, p in zip(m_off, msz, self.pers)] if mode else None)


def _err(got, ref):
    return (got.double() - ref).abs().max().item() if ref.numel() else 0.0


@functools.lru_cache(maxsize=None)
def _scale1(heads, hp, seg):
    """one launch object and its scale-1 results in the three modes, computed once: (job, {mode: (r, maps)})"""
    job = _Launch(seg, MEMBERS, 3, heads, hp, 1000 * heads + hp + seg)  # (token 3: group blocks that are not 16-byte aligned)
    return job, {0: job.target(0), 1: job.target(1, first=8), 2: job.target(2)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. raw C-ABI against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("heads,hp", HEADS)
def test_raw_r_dependency_and_affect_match_float64_row_0(heads, hp, seg):
    job, got = _scale1(heads, hp, seg)
    worst = dict(r=0.0, D=0.0, F=0.0, sums=0.0)
    for g, m in enumerate(MEMBERS):
        D, Fm, R = job.ref[g]
        r, d_t, f_t = got[0][0][g], got[1][1][g], got[2][1][g].view(m, seg)
        assert torch.equal(r, got[1][0][g]) and torch.equal(r, got[2][0][g]), "r differs between the modes"
        worst["r"] = max(worst["r"], _err(r, R[0]))
        worst["D"] = max(worst["D"], _err(d_t, D[0]))
        worst["F"] = max(worst["F"], _err(f_t, Fm[:, :seg]))
        worst["sums"] = max(worst["sums"], abs(r.double().sum().item() - 1), abs(d_t.double().sum().item() - 1),
                            (f_t.double().sum(0) - 1).abs().max().item())
        if m == 1:
            assert abs(r.item() - 1) <= TOL
    print("heads=%d hp=%d seg=%d: max-abs vs float64 r %.2e D_t %.2e F_t %.2e, sum identities %.2e" % (heads, hp, seg, worst["r"], worst["D"], worst["F"], worst["sums"]))
    for name, e in worst.items():
        assert e <= TOL, "heads=%d hp=%d seg=%d: %s max-abs %.2e" % (heads, hp, seg, name, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. agreement with the person form; up-sampling
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("heads,hp", HEADS)
def test_raw_scale_1_is_bit_identical_to_row_0_of_the_person_form(heads, hp, seg):
    job, got = _scale1(heads, hp, seg)
    R, Dp = job.person(1)
    _, Fp = job.person(2)
    for g, m in enumerate(MEMBERS):
        assert torch.equal(got[0][0][g], R[g][0]), "r of group %d is not R[0, :]" % g
        assert torch.equal(got[1][1][g], Dp[g][0]), "D_t of group %d is not D[0, :]" % g
        assert torch.equal(got[2][1][g].view(m, seg), Fp[g][:, :seg]), "F_t of group %d is not F[:, 0:seg]" % g
    again = job.target(2)
    assert all(torch.equal(a, b) for a, b in zip(again[0] + again[1], got[2][0] + got[2][1])), "two runs differ"


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("h,w", [(4, 3), (8, 6)])
def test_raw_upsampling_matches_float64_interpolate(h, w, scale):
    seg = h * w
    for heads, hp in ((2, 48), (1, 80)):
        job, got = _scale1(heads, hp, seg)
        for mode in (1, 2):
            r, M = job.target(mode, scale=scale, h=h, w=w, first=7 if mode == 1 else 4)
            for g, m in enumerate(MEMBERS):
                D, Fm, _ = job.ref[g]
                raw = D[0] if mode == 1 else Fm[:, :seg]
                want = F.interpolate(raw.reshape(1, m, h, w), scale_factor=scale, mode="bilinear", align_corners=False)[0]
                assert M[g].numel() == want.numel() == m * seg * scale * scale
                err = _err(M[g].view(want.shape), want)
                print("x%d %dx%d heads=%d mode %d group %d: max-abs %.2e" % (scale, h, w, heads, mode, g, err))
                assert err <= TOL, "x%d heads=%d mode %d group %d: max-abs %.2e" % (scale, heads, mode, g, err)
                assert torch.equal(r[g], got[0][0][g]), "r changed with the scale"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. canaries: n_grp smaller than the table, an empty group in the middle (every launch checks its buffers in _Launch.target)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,h,w", [(12, 4, 3), (5, 5, 1), (192, 16, 12)])
def test_only_the_first_n_grp_groups_are_written_and_an_empty_group_is_skipped(seg, h, w):
    for heads, hp in ((2, 48), (1, 80)):
        job = _Launch(seg, [2, 0, 3, 2], 1, heads, hp, 31 + seg + hp)
        for mode, scale in ((0, 1), (1, 1), (2, 1), (1, 2), (2, 2)):
            full = job.target(mode, scale, h, w)           # every group of the table; group 1 is empty
            assert full[0][1].numel() == 0
            for n_grp in (3, 1):
                part = job.target(mode, scale, h, w, n_grp=n_grp)
                assert len(part[0]) == n_grp
                for g in range(n_grp):
                    assert torch.equal(part[0][g], full[0][g]) and (not mode or torch.equal(part[1][g], full[1][g]))
            D, Fm, R = job.ref[2]
            assert _err(full[0][2], R[0]) <= TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. bad arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_raw_rejects_bad_arguments():
    L = cabi.lib()
    assert L.i2r_attn_target_maps(None, None) == -1 and b"null pointer" in L.i2r_last_error()
    assert L.i2r_attn_target_maps(ctypes.byref(cabi.AttnTargetArgs()), None) == -1 and b"null pointer" in L.i2r_last_error()
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int64, device="cuda")
    host_off = (ctypes.c_int32 * 3)(0, 10, 300)

    def args(**kw):
        d = dict(qk=buf.data_ptr(), grp_off=ibuf.data_ptr(), ws=buf.data_ptr(), rel=buf.data_ptr(), rel_off=ibuf.data_ptr(), maps=buf.data_ptr(),
                 maps_off=ibuf.data_ptr(), rows=buf.data_ptr(), grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=1, heads=1, hp=16,
                 k_off=16, qk_cs=32, ws_stride=2, seg=5, mode=1, scale=1, h=1, w=1)
        d.update(kw)
        return cabi.AttnTargetArgs(**d)

    for ptr in ("qk", "grp_off", "ws", "rel", "rel_off", "rows", "grp_off_host", "maps", "maps_off"):
        assert L.i2r_attn_target_maps(ctypes.byref(args(**{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    for kw, msg in ((dict(mode=3), b"mode=3"), (dict(mode=-1), b"mode=-1"), (dict(scale=0), b"scale=0"), (dict(scale=65), b"scale=65"),
                    (dict(seg=0), b"seg=0"), (dict(seg=-2), b"seg=-2"), (dict(seg=3), b"not a multiple of seg"), (dict(seg=4), b"not a multiple of seg"),
                    (dict(scale=2, h=2, w=2), b"is not h w"), (dict(scale=2, h=0, w=5), b"is not h w"), (dict(scale=2, h=5, w=1, mode=0, seg=10), b"is not h w"),
                    (dict(heads=0), b"heads=0"), (dict(hp=24, k_off=24, qk_cs=48), b"hp=24"), (dict(hp=272, k_off=272, qk_cs=544), b"hp=272"),
                    (dict(k_off=8), b"row stride"), (dict(k_off=18, qk_cs=36), b"row stride"), (dict(qk_cs=28), b"row stride"), (dict(qk_cs=34), b"row stride"),
                    (dict(qk=buf.data_ptr() + 4), b"alignment"), (dict(ws=buf.data_ptr() + 4), b"alignment"),
                    (dict(ws_stride=3), b"ws_stride=3"), (dict(ws_stride=0), b"ws_stride=0"), (dict(heads=2, k_off=32, qk_cs=64), b"ws_stride=2"),
                    (dict(n_grp=2, ws_stride=4), b"ws_stride=4"),  # the second group has 290 tokens: three key blocks
                    (dict(n_grp=0), b"n_grp=0"), (dict(n_grp=65536), b"n_grp=65536")):
        assert L.i2r_attn_target_maps(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    torch.cuda.synchronize()
    assert not buf.any(), "a rejected call launched something"


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. - 7. through main_target_relations
# ---------------------------------------------------------------------------------------------------------------------------------
def _net(cfg, sd, precision="fp32"):
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    if precision != "fp32":
        net.set_precision(precision)
    return net.cuda()


def _boxes(n, seed=0):
    """top-left corners with distinct distances"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 4, generator=g, dtype=torch.float64) * 200).numpy()


def _multi(y):
    return y["multi"] if isinstance(y, dict) else y


@functools.lru_cache(maxsize=None)
def _expanded(tag, max_patch, kind, up, seed=0):
    """person_relations on the expanded batch (x[members], pos_mask[members], group_len) -- code that predates the target form -- computed
    once, never modified: (members [G] on the host, group_len, result)"""
    cfg, sd, x, m, length, _ = setup(tag)
    net = _net(cfg, sd)
    groups = i2r_input.main_target_groups(_boxes(sum(length), seed), length, max_patch, "cuda")
    idx = groups.members.long()
    _, res = net.person_relations(x.cuda()[idx], m.cuda()[idx], groups.group_len, maps=kind, upsample=up)
    torch.cuda.synchronize()
    return groups.members.cpu(), groups.group_len, res


CASES = [("w48_l31", None, "the tower seam"), ("tph_l21", None, "the expanded batch"), ("tph_l21", True, "the shared first stage")]


@pytest.mark.parametrize("max_patch", [2, 3])
@pytest.mark.parametrize("tag,share,what", CASES)
def test_main_target_relations_match_forward_main_target_and_person_relations_on_the_expanded_batch(tag, share, what, max_patch):
    cfg, sd, x, m, length, _ = setup(tag)
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    xd, md, S = x.cuda(), m.cuda(), sum(length)
    boxes = _boxes(S)
    y0 = net.forward_main_target(xd, md, length, boxes, max_patch=max_patch, share_first_stage=share).clone()
    mode = eng._groups_shared(x.shape[2], x.shape[3], share)
    assert mode == {"the tower seam": "tower", "the expanded batch": None, "the shared first stage": "first"}[what]
    tol = TOL if mode is None else TOL_MODEL
    for kind in (None, "dependency", "affect"):
        for up in ((False,) if kind is None else (False, True)):
            y, res = net.main_target_relations(xd, md, length, boxes, max_patch=max_patch, maps=kind, upsample=up, share_first_stage=share)
            torch.cuda.synchronize()
            assert torch.equal(y, y0), "main_target_relations' heat maps differ from forward_main_target's"
            members, glen, ref = _expanded(tag, max_patch, kind, up)
            # the tables
            want = torch.full((S, max_patch), -1, dtype=torch.int32)
            o = 0
            for g, n in enumerate(glen):
                want[g, :n] = members[o:o + n]
                o += n
            assert res.members.dtype == torch.int32 and torch.equal(res.members.cpu(), want)
            assert res.group_len.dtype == torch.int32 and res.group_len.tolist() == glen and len(glen) == S
            assert set(res.relation) == {(st, l) for l in range(n_layers)} and set(res.maps) == (set(res.relation) if kind else set())
            assert set(res.image_relation) == set(res.relation)
            store = res.relation[(st, 0)].untyped_storage().data_ptr()
            worst = 0.0
            for l in range(n_layers):
                r = res.relation[(st, l)]
                assert r.shape == (S, max_patch) and r.untyped_storage().data_ptr() == store
                assert (r.double().sum(1) - 1).abs().max().item() <= TOL
                errs = []
                for g, n in enumerate(glen):
                    assert not r[g, n:].any(), "a relation entry behind the group"
                    errs.append(_err(r[g, :n], ref.relation[(st, l)][g][0].double()))
                    if kind:
                        mp = res.maps[(st, l)]
                        assert mp.shape[:2] == (S, max_patch) and mp.untyped_storage().data_ptr() == store
                        assert mp[g, :n].shape == ref.maps[(st, l)][g][0].shape
                        assert not mp[g, n:].any(), "a map behind the group"
                        if kind == "dependency":  # D[0]: where the target looks on member s
                            errs.append(_err(mp[g, :n], ref.maps[(st, l)][g][0].double()))
                        else:                     # F[s][target]: which of the target's tokens look at member s
                            errs.append(_err(mp[g, :n], ref.maps[(st, l)][g][:, 0].double()))
                print("%s (%s) max_patch %d maps=%s upsample=%s layer %d: max-abs vs person_relations on the expanded batch %.2e"
                      % (tag, what, max_patch, kind, up, l, max(errs)))
                worst = max(worst, *errs)
            assert worst <= tol, "%s (%s) max_patch %d maps=%s upsample=%s: max-abs %.2e > %.0e" % (tag, what, max_patch, kind, up, worst, tol)
    # max_patch >= max(length): every group holds its whole image, permuted -> the image's relation matrix
    if max_patch >= max(length):
        _, full = net.person_relations(xd, md, length)
        _, res = net.main_target_relations(xd, md, length, boxes, max_patch=max_patch, share_first_stage=share)
        torch.cuda.synchronize()
        for l in range(n_layers):
            for b, n in enumerate(length):
                got = res.image_relation[(st, l)][b]
                assert got.shape == (n, n)
                err = _err(got, full.relation[(st, l)][b].double())
                print("%s (%s) max_patch %d layer %d image %d: image_relation vs person_relations max-abs %.2e" % (tag, what, max_patch, l, b, err))
                assert err <= TOL_MODEL
    else:
        _, res = net.main_target_relations(xd, md, length, boxes, max_patch=max_patch, share_first_stage=share)
        for l in range(n_layers):
            for b, n in enumerate(length):
                got = res.image_relation[(st, l)][b]
                assert got.shape == (n, n) and (got.double().sum(1) - 1).abs().max().item() <= TOL
                assert ((got > 0).sum(1) <= max_patch).all()


@pytest.mark.parametrize("tag,share", [("w48_l31", None), ("tph_l21", None), ("tph_l21", True)])
def test_other_boxes_at_the_same_capacities_build_nothing_and_the_default_grouped_program_is_untouched(tag, share):
    cfg, sd, x, m, length, _ = setup(tag)
    net = _net(cfg, sd)
    eng = net.engine()
    xd, md, S = x.cuda(), m.cuda(), sum(length)
    y0 = net.forward_main_target(xd, md, length, _boxes(S), max_patch=2, share_first_stage=share).clone()
    keys0 = list(eng.programs)
    last0 = list(eng.last_programs)
    ops0 = [[(k, lane) for k, lane, _ in P.ops] for P in last0]
    net.main_target_relations(xd, md, length, _boxes(S), max_patch=2, maps="affect", upsample=2, share_first_stage=share)
    key, = [k for k in eng.programs if "targets" in k]
    builds, n_prog, last = eng.n_builds, len(eng.programs), list(eng.last_programs)
    prog = eng.programs[key][0]
    assert cabi.CAPTURE_OP_ATTN_TARGET in [k for k, _, _ in prog.ops] and prog in last
    for seed in (1, 2):  # other boxes, other neighbours: the same capacities
        _, res = net.main_target_relations(xd, md, length, _boxes(S, seed), max_patch=2, maps="affect", upsample=2, share_first_stage=share)
        torch.cuda.synchronize()
        assert eng.n_builds == builds and len(eng.programs) == n_prog, "a regroup at the same capacities built a program"
        assert len(eng.last_programs) == len(last) and all(a is b for a, b in zip(eng.last_programs, last))
        members, glen, ref = _expanded(tag, 2, "affect", 2, seed)
        assert torch.equal(res.members.cpu()[:, :1].view(-1), torch.arange(S, dtype=torch.int32)), "every person is its own group's target"
        st = eng.inter_stack
        for g, n in enumerate(glen):
            assert _err(res.relation[(st, 0)][g, :n], ref.relation[(st, 0)][g][0].double()) <= TOL_MODEL
    # the default grouped forward still runs its own, untouched programs
    y1 = net.forward_main_target(xd, md, length, _boxes(S), max_patch=2, share_first_stage=share)
    assert eng.n_builds == builds and torch.equal(y1, y0)
    assert len(eng.last_programs) == len(last0) and all(a is b for a, b in zip(eng.last_programs, last0))
    assert [[(k, lane) for k, lane, _ in P.ops] for P in eng.last_programs] == ops0, "the default program's launch list changed"
    assert all(cabi.CAPTURE_OP_ATTN_TARGET not in [k for k, _ in ops] for ops in ops0)
    assert [k for k in eng.programs if "targets" not in k] == [k for k in keys0 if k in eng.programs] and set(keys0) <= set(eng.programs)


def test_bf16_shared_first_stage_heat_maps_are_forward_main_targets_and_the_identities_hold():
    cfg, sd, x, m, length, _ = setup("tph_l21")
    net = _net(cfg, sd, "bf16")
    eng = net.engine()
    st, n_layers = eng.inter_stack, eng.capture_stacks()[eng.inter_stack]
    xd, md, S = x.cuda(), m.cuda(), sum(length)
    boxes = _boxes(S)
    y0 = net.forward_main_target(xd, md, length, boxes, max_patch=2, share_first_stage=True).clone()
    for kind in ("dependency", "affect"):
        y, res = net.main_target_relations(xd, md, length, boxes, max_patch=2, maps=kind, share_first_stage=True)
        torch.cuda.synchronize()
        assert torch.equal(y, y0), "bf16: the heat maps differ from forward_main_target's"
        glen = res.group_len.tolist()
        for l in range(n_layers):
            r, mp = res.relation[(st, l)], res.maps[(st, l)]
            assert torch.isfinite(r).all() and torch.isfinite(mp).all()
            sums = [(r.double().sum(1) - 1).abs().max().item()]
            for g, n in enumerate(glen):
                v = mp[g, :n].double()
                sums.append(abs(v.sum().item() - 1) if kind == "dependency" else (v.sum(0) - 1).abs().max().item())
            print("tph_l21 bf16 maps=%s layer %d: sum identities %.2e" % (kind, l, max(sums)))
            assert max(sums) <= 1e-5
