"""-m gpu: attention maps at query points on the MI355X -- the raw i2r_attn_query_maps C-ABI (rows, columns, up-sampling, bad arguments)
against float64 torch, net.attention_at of every model kind against the CPU restatement (tests/_attn_ref.py) and the reference's own hook
rows (tests/golden/attn_*.npz), consistency with the full capture (fp32 and the 16-bit modes), program reuse and non-interference."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from _attn_query_ref import point_of_token, query_maps
from _attn_ref import restate
from _golden import GOLDEN, keys_manifest, setup
from i2r_amd import arch, cabi, config, models, synth
from i2r_amd.engine import AttnQueries
from i2r_amd.models._base import group_tokens, points_to_tokens

pytestmark = pytest.mark.gpu
TOL = 1e-3
CANARY = 12345.0
LENS = [17, 768, 1, 3072, 5, 192, 1152, 16]


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------------------
# raw C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def _make_qk(heads, hp, lens, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    hd = hp - 3 if hp > 16 else hp  # (pad dims of the head stay exactly 0)
    hs = heads * hp
    k_off = hs + 16
    qk_cs = k_off + hs + 8
    n_tok = sum(lens)
    qk = torch.zeros(n_tok, qk_cs, device="cuda")
    for h in range(heads):
        qk[:, h * hp:h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g) * 2.0 * hd ** -0.5
        qk[:, k_off + h * hp:k_off + h * hp + hd] = torch.randn(n_tok, hd, device="cuda", generator=g)
    return qk, k_off, qk_cs


def _full_maps(qk, heads, hp, k_off, lens):
    """float64 [L, L] head-averaged maps of the groups (the reference of tests/test_attn_maps_gpu.py)"""
    out, o = [], 0
    for n in lens:
        q = qk[o:o + n].double()
        ref = torch.zeros(n, n, dtype=torch.float64, device="cuda")
        for h in range(heads):
            ref += torch.softmax(q[:, h * hp:(h + 1) * hp] @ q[:, k_off + h * hp:k_off + (h + 1) * hp].t(), dim=-1)
        out.append(ref / heads)
        o += n
    return out


def _token_table(lens, K, seed):
    """[groups, K]: every row holds 0, L - 1, a duplicate and a -1 when it has room for them (K = 1: one of them, by turns)"""
    rng = np.random.RandomState(seed)
    tab = np.zeros((len(lens), K), dtype=np.int32)
    for gi, n in enumerate(lens):
        special = [0, n - 1, -1, n // 2, n // 2]
        row = special[gi % 3:gi % 3 + 1] if K == 1 else (special + list(rng.randint(0, n, size=max(K - 5, 0))))[:K]
        tab[gi] = rng.permutation(row) if K > 1 else row
    return tab


def _run_query(qk, heads, hp, k_off, qk_cs, lens, n_grp, tab, mode, scale=1, h=1, w=1, counts=None, first=7, gap=5):
    """one i2r_attn_query_maps call over the first n_grp groups into blocks separated by canary gaps -> (out, block offsets, block sizes)"""
    K = tab.shape[1]
    cnt = list(counts) if counts is not None else [K] * n_grp
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    out_off, sizes, pos = [], [], first
    for n, c in zip(lens[:n_grp], cnt):
        out_off.append(pos)
        sizes.append(c * n * scale * scale)
        pos += sizes[-1] + gap
    out = torch.full((pos + 64,), CANARY, device="cuda")
    goff = torch.tensor(offs, dtype=torch.int32, device="cuda")
    ooff = torch.tensor(out_off, dtype=torch.int64, device="cuda")
    nkb = max(-(-n // 128) for n in lens[:n_grp])
    stride = 2 * heads * nkb
    ws = torch.empty(stride * (n_grp * K if mode == 0 else offs[n_grp]), device="cuda")
    rows = torch.full((K * offs[n_grp] + 8,), CANARY, device="cuda")
    d_tab = torch.from_numpy(np.ascontiguousarray(tab)).cuda()
    d_cnt = torch.tensor(cnt, dtype=torch.int32, device="cuda") if counts is not None else None
    host_off = (ctypes.c_int32 * (n_grp + 1))(*offs[:n_grp + 1])
    if mode == 0:
        tiles, col_tiles = sum(-(-c // 16) * -(-n // 128) for n, c in zip(lens, cnt)), 0
    else:
        tiles = sum(-(-n // 16) * -(-n // 128) for n in lens[:n_grp])
        col_tiles = sum(-(-n // 16) * -(-c // 16) for n, c in zip(lens, cnt))
    a = cabi.AttnQueryArgs(qk=qk.data_ptr(), out=out.data_ptr(), grp_off=goff.data_ptr(), out_off=ooff.data_ptr(), ws=ws.data_ptr(),
                           q_tok=d_tab.data_ptr(), q_cnt=d_cnt.data_ptr() if d_cnt is not None else None, rows=rows.data_ptr(),
                           grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=n_grp, heads=heads, hp=hp, k_off=k_off, qk_cs=qk_cs,
                           n_tiles=tiles, ws_stride=stride, mode=mode, K=K, scale=scale, h=h, w=w, n_col_tiles=col_tiles)
    cabi.check(cabi.lib().i2r_attn_query_maps(ctypes.byref(a), _stream()), "i2r_attn_query_maps")
    torch.cuda.synchronize()
    assert (rows[K * offs[n_grp]:] == CANARY).all(), "a store behind the rows workspace"
    return out, out_off, sizes


def _check_canaries(out, out_off, sizes):
    written = torch.zeros(out.numel(), dtype=torch.bool, device="cuda")
    for o, n in zip(out_off, sizes):
        written[o:o + n] = True
    assert (out[~written] == CANARY).all(), "a store outside the computed blocks"


@pytest.mark.parametrize("heads,hp", [(1, 96), (1, 80), (2, 48), (4, 32), (8, 16)])
def test_raw_rows_and_columns_match_float64(heads, hp):
    lens = LENS + [40]  # the last group is in the offset table but not computed (n_grp excludes it)
    qk, k_off, qk_cs = _make_qk(heads, hp, lens, heads * 1000 + hp)
    full = _full_maps(qk, heads, hp, k_off, LENS)
    cases = [(K, mode, None) for K in (1, 17, 33) for mode in (0, 1)]
    cases += [(33, mode, [33, 1, 20, 17, 2, 33, 16, 5]) for mode in (0, 1)]  # q_cnt: group g uses its first entries only
    for K, mode, counts in cases:
        tab = _token_table(LENS, K, 100 * K + mode)
        # (offsets not all multiples of 4: both store forms; K = 17: a first block at a multiple of 4 as well)
        out, out_off, sizes = _run_query(qk, heads, hp, k_off, qk_cs, lens, len(LENS), tab, mode, counts=counts, first=8 if K == 17 else 7)
        for gi, n in enumerate(LENS):
            c = counts[gi] if counts is not None else K
            ref = query_maps(full[gi], tab[gi, :c], mode, 1, 1).reshape(c, n)
            got = out[out_off[gi]:out_off[gi] + c * n].view(c, n)
            err = (got.double() - ref).abs().max().item()
            assert err <= 1e-5, "mode %d K=%d L=%d heads=%d hp=%d: max-abs %.2e" % (mode, K, n, heads, hp, err)
            real = torch.from_numpy(tab[gi, :c] >= 0).cuda()
            if mode == 0:
                assert not bool(real.any()) or (got[real].double().sum(-1) - 1).abs().max().item() <= 1e-5
            assert (got[~real] == 0).all(), "a skipped (-1) entry is not exactly 0"
            dup = np.flatnonzero(tab[gi, :c] == n // 2)
            if len(dup) > 1:
                assert torch.equal(got[dup[0]], got[dup[1]]), "duplicate entries differ"
        _check_canaries(out, out_off, sizes)


@pytest.mark.parametrize("P,h,w,scale", [(1, 4, 3, 4), (1, 8, 6, 3), (3, 16, 12, 16), (1, 64, 48, 4), (2, 16, 12, 1)])
def test_raw_upsampling_matches_float64_interpolate(P, h, w, scale):
    heads, hp, K = 2, 32, 5
    lens = [P * h * w, 2 * P * h * w if h * w < 1000 else P * h * w, h * w, 24]  # (the last one is outside n_grp and no multiple of h w)
    qk, k_off, qk_cs = _make_qk(heads, hp, lens, 7 * h + scale)
    full = _full_maps(qk, heads, hp, k_off, lens[:3])
    tab = _token_table(lens[:3], K, scale)
    for mode in (0, 1):
        out, out_off, sizes = _run_query(qk, heads, hp, k_off, qk_cs, lens, 3, tab, mode, scale=scale, h=h, w=w, first=4 if mode else 7)
        for gi, n in enumerate(lens[:3]):
            ref = query_maps(full[gi], tab[gi], mode, h, w, scale)
            got = out[out_off[gi]:out_off[gi] + sizes[gi]].view(ref.shape)
            assert sizes[gi] == ref.numel() == K * n * scale * scale
            err = (got.double() - ref).abs().max().item()
            # bilinear weights are convex: they cannot enlarge the 1e-5 of the rows; 1e-6: four fp32 roundings of values <= 1
            assert err <= 1e-5 + 1e-6, "mode %d P=%d %dx%d x%d group %d: max-abs %.2e" % (mode, P, h, w, scale, gi, err)
            assert (got[torch.from_numpy(tab[gi] < 0).cuda()] == 0).all()
        _check_canaries(out, out_off, sizes)


def _run_full(qk, heads, hp, k_off, qk_cs, lens, first=7, gap=5):
    """one i2r_attn_weights call over the groups into [L, L] blocks separated by canary gaps -> (out, block offsets, block sizes)"""
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    out_off, sizes, pos = [], [], first
    for n in lens:
        out_off.append(pos)
        sizes.append(n * n)
        pos += n * n + gap
    out = torch.full((pos + 64,), CANARY, device="cuda")
    goff = torch.tensor(offs, dtype=torch.int32, device="cuda")
    ooff = torch.tensor(out_off, dtype=torch.int64, device="cuda")
    stride = 2 * heads * max(-(-n // 128) for n in lens)
    ws = torch.empty(stride * offs[-1], device="cuda")
    a = cabi.AttnWeightsArgs(qk.data_ptr(), out.data_ptr(), goff.data_ptr(), ooff.data_ptr(), ws.data_ptr(), len(lens), heads, hp, k_off, qk_cs,
                             sum(-(-n // 16) * -(-n // 128) for n in lens), stride)
    cabi.check(cabi.lib().i2r_attn_weights(ctypes.byref(a), _stream()), "i2r_attn_weights")
    torch.cuda.synchronize()
    return out, out_off, sizes


@pytest.mark.parametrize("heads,hp", [(1, 96), (2, 48), (8, 16)])
def test_identity_rows_equal_the_full_capture_bitwise(heads, hp):
    """Mode 0 with the identity token table IS the full capture: both forms run the same block statistics, combine, block probabilities
    and store tail of csrc/i2r_encoder_mh.hip, so their blocks are torch.equal, not merely close.  Group lengths: one lane, a ragged
    16-tile, an exact tile, a tile plus one, a second key block holding one key, three key blocks with a ragged end.  (The two outputs
    start at 7 and at 8 floats: every block takes the other store form in the other call.)"""
    lens = [1, 5, 16, 17, 129, 260]
    qk, k_off, qk_cs = _make_qk(heads, hp, lens, 31 * heads + hp)
    tab = np.zeros((len(lens), max(lens)), dtype=np.int32)
    for gi, n in enumerate(lens):
        tab[gi, :n] = np.arange(n)
    got, got_off, sizes = _run_query(qk, heads, hp, k_off, qk_cs, lens, len(lens), tab, 0, counts=lens, first=7)
    full, full_off, full_sizes = _run_full(qk, heads, hp, k_off, qk_cs, lens, first=8)
    assert sizes == full_sizes == [n * n for n in lens]
    _check_canaries(got, got_off, sizes)
    _check_canaries(full, full_off, sizes)
    for gi, n in enumerate(lens):
        a, b = got[got_off[gi]:got_off[gi] + n * n], full[full_off[gi]:full_off[gi] + n * n]
        assert not (b == CANARY).any(), "L=%d: an entry of the full capture was not written" % n
        assert torch.equal(a, b), "L=%d heads=%d hp=%d: %d entries differ, max-abs %.2e" % (n, heads, hp, int((a != b).sum()), (a - b).abs().max().item())


def test_raw_rejects_bad_arguments():
    L = cabi.lib()
    a = cabi.AttnQueryArgs()
    assert L.i2r_attn_query_maps(None, None) == -1 and b"null pointer" in L.i2r_last_error()
    assert L.i2r_attn_query_maps(ctypes.byref(a), None) == -1 and b"null pointer" in L.i2r_last_error()
    buf = torch.zeros(4096, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int64, device="cuda")
    host_off = (ctypes.c_int32 * 2)(0, 10)

    def args(**kw):
        d = dict(qk=buf.data_ptr(), out=buf.data_ptr(), grp_off=ibuf.data_ptr(), out_off=ibuf.data_ptr(), ws=buf.data_ptr(), q_tok=ibuf.data_ptr(),
                 rows=buf.data_ptr(), grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=1, heads=1, hp=16, k_off=16, qk_cs=32,
                 n_tiles=1, ws_stride=2, mode=0, K=1, scale=1, h=1, w=1, n_col_tiles=1)
        d.update(kw)
        return cabi.AttnQueryArgs(**d)

    for ptr in ("qk", "out", "grp_off", "out_off", "ws", "q_tok"):
        assert L.i2r_attn_query_maps(ctypes.byref(args(**{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    for ptr in ("rows", "grp_off_host"):  # needed for scale > 1 only
        assert L.i2r_attn_query_maps(ctypes.byref(args(scale=2, h=5, w=2, **{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    for kw, msg in ((dict(mode=2), b"mode=2"), (dict(mode=-1), b"mode=-1"), (dict(scale=0), b"scale=0"), (dict(scale=-3), b"scale=-3"),
                    (dict(K=0), b"K=0"), (dict(K=-1), b"K=-1"), (dict(scale=2, h=3, w=3), b"not a multiple of h w"),
                    (dict(scale=2, h=0, w=3), b"h=0")):
        assert L.i2r_attn_query_maps(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    torch.cuda.synchronize()
    assert not buf.any(), "a rejected call launched something"


# ---------------------------------------------------------------------------------------------------------------------------------
# through attention_at
# ---------------------------------------------------------------------------------------------------------------------------------
def _net(cfg, sd, precision="fp32"):
    net = eval("models." + cfg.MODEL.NAME + ".get_pose_net")(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    if precision != "fp32":
        net.set_precision(precision)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _restated(tag):
    """(cfg, sd, x, m, length, restated maps, stack inputs, fixture or None): computed once per tag, never modified"""
    cfg, sd, x, m, length, _ = setup(tag)
    maps, feats, _ = restate(cfg, sd, x, m, length)
    fpath = os.path.join(GOLDEN, "attn_%s.npz" % tag)
    return cfg, sd, x, m, length, maps, feats, (dict(np.load(fpath)) if os.path.exists(fpath) else None)


def _entry_rows(fx, st, n_layers, b, n, seed):
    """query tokens of batch entry b: the union over the layers of the fixture's hook rows where there are some (the reference recorded
    another row set per layer), else 0, n - 1 and a few seeded ones"""
    if fx is not None and "%s.0.%d.rows" % (st, b) in fx:
        return sorted({int(r) for l in range(n_layers) for r in fx["%s.%d.%d.rows" % (st, l, b)]})
    return sorted({0, n - 1} | {int(v) for v in np.random.RandomState(seed).randint(0, n, size=4)})


def _points_for(rows_per_entry, entries, hw, fw, down):
    """rows_per_entry[b]: group-level tokens of entry b; entries[b]: its crops.  -> (points [S, K, 2] with NaN in the unused slots,
    per entry the result index of each of its rows): row j of an entry is slot j of the crop of its person"""
    K = max(len(r) for r in rows_per_entry)
    S = sum(len(e) for e in entries)
    pts = torch.full((S, K, 2), float("nan"), dtype=torch.float64)
    index = []
    for rows, crops in zip(rows_per_entry, entries):
        idx = []
        for j, r in enumerate(rows):
            person, tok = r // hw, r % hw
            pts[crops[person], j] = torch.tensor(point_of_token(tok, fw, down), dtype=torch.float64)
            idx.append(person * K + j)
        index.append(idx)
    return pts, index, K


def _check_stack(net_call, st, n_layers, intra, length, maps, feats, fx, H, tag):
    """both modes, raw maps, against the restatement and the reference's hook rows; mode 0 also up-sampled to input resolution"""
    fh, fw = feats[st].shape[2:]
    hw, down = fh * fw, H // fh
    S = sum(length)
    if intra:
        entries, lens = [[s] for s in range(S)], [hw] * S
    else:
        starts = np.cumsum([0] + list(length))
        entries, lens = [list(range(starts[b], starts[b + 1])) for b in range(len(length))], [n * hw for n in length]
    rows = [_entry_rows(fx, st, n_layers, b, n, b) for b, n in enumerate(lens)]
    pts, index, K = _points_for(rows, entries, hw, fw, down)
    layers = {(st, i) for i in range(n_layers)}
    worst = 0.0
    for mode, name in ((0, "dependency"), (1, "affect")):
        _, got = net_call(pts, name, layers, False)
        assert set(got) == layers
        for (_, l), res in got.items():
            w_ref = maps[(st, l)]
            for b, n in enumerate(lens):
                g = res[b].cpu()
                assert g.shape == ((K, 1, fh, fw) if intra else (len(entries[b]) * K, len(entries[b]), fh, fw)), (tag, st, l, g.shape)
                sel = g[index[b]].reshape(len(rows[b]), n)
                ref = query_maps(w_ref[b, :n, :n], rows[b], mode, fh, fw).reshape(len(rows[b]), n)
                err = (sel.double() - ref).abs().max().item()
                worst = max(worst, err)
                assert err < TOL, "%s %s.%d entry %d mode %d: max-abs %.2e vs restatement" % (tag, st, l, b, mode, err)
                unused = sorted(set(range(g.shape[0])) - set(index[b]))
                assert not g[unused].any(), "a skipped (NaN) point's map is not exactly 0"
                if fx is not None and "%s.%d.%d.rows" % (st, l, b) in fx:
                    fr = [int(r) for r in fx["%s.%d.%d.rows" % (st, l, b)]]  # this layer's hook rows, as positions in the query set
                    at = [rows[b].index(r) for r in fr]
                    hook = torch.from_numpy(fx["%s.%d.%d.maps" % (st, l, b)])[:, :n]
                    # mode 0: the reference's hook rows; mode 1: column q restricted to the fixture rows = hook[:, q]
                    e2 = (sel[at] - hook).abs().max().item() if mode == 0 else (sel[at][:, fr] - hook[:, fr].t()).abs().max().item()
                    assert e2 < TOL, "%s %s.%d entry %d mode %d: max-abs %.2e vs the reference's hook rows" % (tag, st, l, b, mode, e2)
    _, up = net_call(pts, "dependency", {(st, 0)}, True)  # r = down_rate: input resolution
    for b, n in enumerate(lens):
        g = up[(st, 0)][b].cpu()
        assert g.shape[-2:] == (fh * down, fw * down) and fh * down == H
        ref = query_maps(maps[(st, 0)][b, :n, :n], rows[b], 0, fh, fw, down)
        assert (g[index[b]].double() - ref).abs().max().item() < TOL
    return worst


@pytest.mark.parametrize("tag", ["w48_l31", "tph_l21", "hrt_l21", "w48_nh8_l21", "hrt_pre_nh2_l21"])
def test_attention_at_matches_restatement_and_reference(tag):
    cfg, sd, x, m, length, maps, feats, fx = _restated(tag)
    net = _net(cfg, sd)
    xd, md = x.cuda(), m.cuda()
    call = lambda pts, mode, layers, up: net.attention_at(xd, md, length, pts, mode=mode, layers=layers, upsample=up)  # noqa: E731
    stacks = net.engine().capture_stacks()
    assert set(stacks) == {st for st, _ in maps}
    for st, n_layers in stacks.items():
        worst = _check_stack(call, st, n_layers, st.startswith("singleformer."), length, maps, feats, fx, x.shape[2], tag)
        print("%s %s: max-abs vs restatement %.2e" % (tag, st, worst))
    torch.cuda.synchronize()


@pytest.mark.parametrize("tag", ["tph_l21", "hrt_pre_nh2_l21"])
def test_attention_at_defaults_return_every_stack_at_input_resolution(tag):
    """layers=None, upsample=True: every layer of every stack in ONE call, each stack up-sampled by its own down_rate (4 for the
    intra-human, 16 for the inter-human stack of a 256 x 192 model), against float64 F.interpolate of the restatement's rows / columns"""
    cfg, sd, x, m, length, maps, feats, _ = _restated(tag)
    net = _net(cfg, sd)
    H, W = x.shape[2:]
    S, K = sum(length), 3
    rng = np.random.RandomState(11)
    pts = torch.from_numpy(np.stack([rng.uniform(0, W, size=(S, K)), rng.uniform(0, H, size=(S, K))], -1))
    pts[0, 1] = float("nan")
    for mode, name in ((0, "dependency"), (1, "affect")):
        kw = {} if mode == 0 else {"mode": name}
        out, got = net.attention_at(x.cuda(), m.cuda(), length, pts, **kw)
        torch.cuda.synchronize()
        assert set(got) == set(maps) and len({st for st, _ in got}) == len(feats)
        for (st, l), res in got.items():
            fh, fw = feats[st].shape[2:]
            tok = points_to_tokens(pts, H, W, fh, fw)
            if st.startswith("singleformer."):
                assert tuple(res.shape) == (S, K, 1, H, W)
                tabs, lens, res = list(tok), [fh * fw] * S, list(res)
            else:
                table, counts = group_tokens(tok, length, fh * fw)
                tabs, lens = [table[b, :c] for b, c in enumerate(counts)], [n * fh * fw for n in length]
            for b, n in enumerate(lens):
                ref = query_maps(maps[(st, l)][b, :n, :n], tabs[b], mode, fh, fw, H // fh)
                assert tuple(res[b].shape) == tuple(ref.shape) and ref.shape[-2:] == (H, W), (tag, st, l, res[b].shape)
                err = (res[b].cpu().double() - ref).abs().max().item()
                assert err < TOL, "%s %s.%d entry %d mode %d: max-abs %.2e" % (tag, st, l, b, mode, err)
        assert not got[(sorted(feats)[-1], 0)][0][1].any(), "the NaN point's map is not exactly 0"


def test_attention_at_standalone_transpose_h():
    cfg = config.load_config("tph_192_p6_b4")
    sd = synth.make_state_dict(arch.transpose_h_spec(cfg, ""))
    net = models.transpose_h.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    x, _, _ = synth.make_inputs([2, 1], 256, 192)
    maps, feats, y = restate(cfg, sd, x, None, None, standalone_single=True)
    xd = x.cuda()
    call = lambda pts, mode, layers, up: net.attention_at(xd, pts, mode=mode, layers=layers, upsample=up)  # noqa: E731
    (feat, hm), _ = call(torch.zeros(3, 1, 2), "dependency", None, True)
    assert (hm.cpu() - y[1]).abs().max().item() < TOL
    worst = _check_stack(call, "global_encoder", cfg.MODEL.ENCODER_LAYERS, True, [2, 1], maps, feats, None, 256, "transpose_h")
    print("transpose_h: max-abs vs restatement %.2e" % worst)


def _tokens_for(eng, length, H, W, K, seed):
    """engine-level query tables of every capture stack: random tokens with 0, the last one and a -1"""
    rng = np.random.RandomState(seed)
    tokens, lens_of = {}, {}
    for st, (fh, fw) in eng.capture_map_sizes(H, W).items():
        single = st == getattr(eng, "single_stack", None)
        lens = [fh * fw] * sum(length) if single else [n * fh * fw for n in length]
        tab = np.stack([rng.randint(0, n, size=K) for n in lens]).astype(np.int32)
        tab[:, 0], tab[:, 1], tab[:, 2] = 0, np.array(lens) - 1, -1
        tokens[st], lens_of[st] = torch.from_numpy(tab), lens
    return tokens, lens_of


@pytest.mark.parametrize("tag,precision", [("w48_l31", "fp32"), ("hrt_pre_nh2_l21", "fp32"), ("tph_l21", "bf16"), ("hrt288_l2", "fp16")])
def test_query_maps_equal_rows_and_columns_of_the_full_capture(tag, precision):
    """scale 1: the query maps are the same rows / columns of forward(capture=)'s maps within 2e-5 (each side is within 1e-5 of exact) --
    on the fused layers' fp32 re-projection (fp32 and 16-bit) and on the general layer's own q|k activation (hrt_pre_nh2)"""
    cfg, sd, x, m, length, _ = setup(tag)
    net = _net(cfg, sd, precision)
    eng = net.engine()
    capture = {(st, i) for st, n in eng.capture_stacks().items() for i in range(n)}
    xd, md = x.cuda(), m.cuda()
    y_full, full = eng.forward(xd, md, length, capture=capture)
    tokens, lens_of = _tokens_for(eng, length, x.shape[2], x.shape[3], 19, 5)
    for mode in (0, 1):
        y_q, got = eng.forward(xd, md, length, capture=capture, queries=AttnQueries(tokens, mode, 1))
        torch.cuda.synchronize()
        for key in capture:
            fh, fw = eng.capture_map_sizes(x.shape[2], x.shape[3])[key[0]]
            for b, n in enumerate(lens_of[key[0]]):
                ref = query_maps(full[key][b], tokens[key[0]][b], mode, fh, fw)
                assert got[key][b].shape == ref.shape
                err = (got[key][b].double() - ref).abs().max().item()
                assert err <= 2e-5, "%s %s %s entry %d mode %d: max-abs %.2e vs the full capture" % (tag, precision, key, b, mode, err)
        ya, yb = (y_full["multi"], y_q["multi"]) if isinstance(y_full, dict) else (y_full, y_q)
        assert torch.equal(ya, yb)


def test_new_points_and_regroup_reuse_one_program():
    """length [4, 4, 3] (capacity 12: one padding slot), new points, then [1, 2, 3, 5]: one program, every result right, and the capture
    buffer holds exactly sum over layers and groups of K_g L_g r^2 floats"""
    cfg = config.load_config("w48_pure_en6")
    sd = synth.make_state_dict([(k, s, d) for k, (s, d) in keys_manifest("w48_pure_en6").items()])
    net = _net(cfg, sd)
    eng = net.engine()
    st, n_layers, K, r, hw, fw = "global_encoder", cfg.MODEL.ENCODER_LAYERS, 3, 2, 192, 12
    layers = {(st, i) for i in range(n_layers)}
    builds, prog, seen = None, None, []
    for i, (length, seed) in enumerate((([4, 4, 3], 0), ([4, 4, 3], 1), ([1, 2, 3, 5], 2))):
        x, m, length = synth.make_inputs(length, 256, 192)
        xd, md = x.cuda(), m.cuda()
        S = sum(length)
        tok = torch.from_numpy(np.random.RandomState(seed).randint(0, hw, size=(S, K)))
        pts = torch.tensor([[point_of_token(int(t), fw, 16) for t in row] for row in tok])
        _, got = net.attention_at(xd, md, length, pts, mode="affect", layers=layers, upsample=r)
        torch.cuda.synchronize()
        key = next(k for k in eng.programs if "query" in k)
        if i == 0:
            prog = eng.programs[key][0]
        else:
            assert eng.n_builds == builds and eng.programs[key][0] is prog, "new points or a regroup at the same capacity rebuilt the program"
        assert sum(1 for k in eng.programs if "query" in k) == 1
        # the buffer: a condition on its shape
        storage = got[(st, 0)][0].untyped_storage().nbytes() // 4
        assert storage == n_layers * sum((n * K) * (n * hw) * r * r for n in length), (storage, length)
        seen.append(torch.cat([v.reshape(-1) for v in got[(st, n_layers - 1)]]).clone())
        # right: against the full capture of the same inputs (itself checked against the restatement in tests/test_attn_maps_gpu.py)
        _, full = eng.forward(xd, md, length, capture=layers)
        if i == 0:
            builds = eng.n_builds  # (the full capture is a program of its own, built once as well)
        assert eng.n_builds == builds and eng.programs[key][0] is prog
        s0 = 0
        for b, n in enumerate(length):
            table = torch.cat([tok[s0 + p] + p * hw for p in range(n)])
            for l in range(n_layers):
                ref = query_maps(full[(st, l)][b], table, 1, 16, 12, r)
                assert got[(st, l)][b].shape == (n * K, n, 16 * r, 12 * r)
                assert (got[(st, l)][b].double() - ref).abs().max().item() <= 2e-5 + 1e-6
            s0 += n
    assert not torch.equal(seen[0], seen[1]) and seen[1].shape != seen[2].shape


def test_attention_at_does_not_interfere():
    cfg = config.load_config("w48_pure_en6")
    sd = synth.make_state_dict([(k, s, d) for k, (s, d) in keys_manifest("w48_pure_en6").items()])
    net = _net(cfg, sd)
    x, m, length = synth.make_inputs([2, 1], 256, 192)
    xd, md = x.cuda(), m.cuda()
    eng = net.engine()
    y0 = net(xd, md, length).clone()
    rec = {}
    hooks = [net.global_encoder.layers[i].self_attn.register_forward_hook(lambda mod, inp, out, i=i: rec.setdefault(i, []).append(out[1])) for i in (0, 5)]
    yh = net(xd, md, length).clone()
    keys0 = set(eng.programs)
    assert len(keys0) == 2 and sum(1 for k in keys0 if "capture" in k) == 1
    pts = torch.tensor([[[10.0, 20.0], [float("nan"), 0.0]]] * 3)
    ya, got = net.attention_at(xd, md, length, pts)
    torch.cuda.synchronize()
    assert torch.equal(ya, y0), "attention_at's heat maps differ from the default forward's"
    assert set(got) == {("global_encoder", i) for i in range(6)}
    assert keys0 < set(eng.programs) and len(eng.programs) == len(keys0) + 1, "the default / full-capture programs left the cache"
    assert all(len(v) == 1 for v in rec.values()), "attention_at served forward hooks"
    builds = eng.n_builds
    y1 = net(xd, md, length).clone()  # still hooked: the full maps, on the program cached before
    assert eng.n_builds == builds and torch.equal(y1, yh)
    for i in (0, 5):
        assert len(rec[i]) == 2 and rec[i][1].shape == (2, 2 * 192, 2 * 192) and torch.equal(rec[i][0], rec[i][1])
        # and the query maps are rows of what the hooks got
        row = rec[i][1][0, (20 // 16) * 12 + 10 // 16, :2 * 192]
        assert got[("global_encoder", i)][0].shape == (2 * 2, 2, 256, 192) and got[("global_encoder", i)][1].shape == (2, 1, 256, 192)
        raw = net.attention_at(xd, md, length, pts, layers={("global_encoder", i)}, upsample=False)[1][("global_encoder", i)][0][0]
        assert (raw.reshape(-1) - row).abs().max().item() <= 2e-5
    for h in hooks:
        h.remove()
    assert torch.equal(net(xd, md, length), y0)
    with pytest.raises(ValueError):
        net.attention_at(xd, md, length, torch.tensor([[[192.0, 0.0]]] * 3))
    with pytest.raises(ValueError):
        eng.forward(xd, md, length, capture={("global_encoder", 0)}, queries=AttnQueries({"global_encoder": torch.tensor([[384], [0]])}))
