"""-m gpu: i2r_val_combine (the loss / PCK accuracy of a whole batch from the raw sums of its data-parallel shards) through the raw C-ABI
with canaries around every output, against the numpy restatement tests/_val_combine_ref.py; one part against i2r_val_metrics itself, bit
for bit; the reference's own output (tests/golden/val_metrics_reference.npz) cut into shards on the device; behind the model; through an
RCCL group of one rank; and caller.PoseTable against one oks_eval call."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _val_combine_ref as cref
import _val_ref
from _golden import setup
from _oks_cases import coco_dict, draw_image
from i2r_amd import cabi, caller, models
from i2r_amd import dist as i2r_dist
from test_val_combine import SHARDED
from test_val_metrics import case, restated
from test_val_metrics_gpu import CANARY, GUARD, SUM_RTOL, Guarded, analytic_loss_bound, dev, up

pytestmark = pytest.mark.gpu

F64, I32 = torch.float64, torch.int32
OUTS = (("sse", F64, 0), ("hits", I32, 0), ("valid", I32, 0), ("loss", F64, None), ("acc", F64, 1), ("avg_acc", F64, None), ("cnt", I32, None),
        ("n_crops", I32, None))   # (name, dtype, elements = joints + this, or 1)


def bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def run_combine(parts, J, h, w, meter=None, expect=0, bad=None):
    """the raw C-ABI call; parts numpy [n_part, 1 + 3 J] -> (dict of numpy outputs with the canaries checked | None, the Guarded buffers)"""
    p = up(parts, np.float64)
    o = {n: Guarded(1 if k is None else J + k, dt) for n, dt, k in OUTS}
    a = cabi.ValCombineArgs(parts=p.data_ptr(), meter=meter, n_part=parts.shape[0], joints=J, h=h, w=w, **{n: g.ptr() for n, g in o.items()})
    for k, v in (bad or {}).items():      # fields overwritten after the fact: bad arguments
        setattr(a, k, v)
    rc = cabi.lib().i2r_val_combine(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    torch.cuda.synchronize()
    return ({n: g.get().copy() for n, g in o.items()} if expect == 0 else None), o


def guarded_meter(values):
    t = torch.full((4 + 2 * GUARD,), CANARY[F64], dtype=F64, device=dev())
    t[GUARD:GUARD + 4] = torch.tensor(values, dtype=F64)
    return t


def meter_of(t):
    a = t.cpu().numpy()
    assert (a[:GUARD] == CANARY[F64]).all() and (a[-GUARD:] == CANARY[F64]).all(), "canary overwritten"
    return a[GUARD:-GUARD]


def draw_parts(rng, n_part, J):
    """rows as val_metrics' raw sums look: n crops, valid <= n, hits <= valid, sse >= 0 of very different sizes; about a third of the
    parts has no crop, and such a row holds numbers that must not be read; one n_crops is negative"""
    parts = np.zeros((n_part, 1 + 3 * J))
    for r in range(n_part):
        n = int(rng.integers(1, 40)) if n_part == 1 or rng.random() > 0.35 else 0
        valid = rng.integers(0, n + 1, J) if n else rng.integers(0, 9, J)
        valid[rng.random(J) < 0.2] = 0
        parts[r, 0] = n
        parts[r, 1:1 + J] = rng.random(J) * 10.0 ** rng.integers(-6, 4, J)
        parts[r, 1 + J:1 + 2 * J] = rng.integers(0, valid + 1)
        parts[r, 1 + 2 * J:] = valid
    if n_part > 1:
        parts[0 if n_part == 2 else n_part // 2, 0] = -3.0
        parts[1, 0] = max(parts[1, 0], 1.0)      # (at least one part with crops, and one joint that counts)
        parts[1, 1 + J], parts[1, 1 + 2 * J] = min(parts[1, 1 + J], 1.0), 1.0
    return parts


def check_against_restatement(got, want, what):
    for n in ("hits", "valid"):
        assert np.array_equal(got[n], getattr(want, n)), (what, n)
    assert got["n_crops"][0] == want.n_crops and got["cnt"][0] == want.cnt, what
    assert np.array_equal(bits(got["acc"]), bits(want.acc)) and bits(got["avg_acc"])[0] == bits(want.avg_acc), (what, got["acc"], want.acc)
    # the order of the additions is part of the entry's statement (ascending part index): the restatement adds in it, IEEE does the rest
    assert np.array_equal(bits(got["sse"]), bits(want.sse)), what
    rel = np.abs(got["sse"] - want.sse) / np.where(want.sse != 0, want.sse, 1.0)
    lrel = abs(got["loss"][0] - want.loss) / (want.loss if want.loss != 0 else 1.0)
    print("%s: sse max rel %.3g, loss rel %.3g (bound %.3g)" % (what, rel.max(), lrel, SUM_RTOL))
    assert (rel <= SUM_RTOL).all() and lrel <= SUM_RTOL, (what, rel.max(), lrel)


# ---- the raw C-ABI against the numpy restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("J", [1, 14, 17, 40])
@pytest.mark.parametrize("n_part", [1, 2, 7, 300])
def test_raw_call_equals_the_restatement(n_part, J):
    """300 parts: more than the workgroup has threads; parts without crops (and one with a negative count) hold numbers that are not read"""
    rng = np.random.default_rng([n_part, J])
    parts = draw_parts(rng, n_part, J)
    assert n_part == 1 or ((parts[:, 0] <= 0).any() and (parts[parts[:, 0] <= 0, 1:] != 0).any())
    h, w = 17, 13
    start = [0.5, 3.0, 1.25, 7.0]
    ref_meter = list(start)
    want = cref.combine(parts, h, w, meter=ref_meter)
    m = guarded_meter(start)
    got, _ = run_combine(parts, J, h, w, meter=m.data_ptr() + 8 * GUARD)
    check_against_restatement(got, want, "%d parts, %d joints" % (n_part, J))
    got_m = meter_of(m)
    assert got_m[1] == ref_meter[1] and got_m[3] == ref_meter[3] and got_m[2] == ref_meter[2]
    assert abs(got_m[0] - ref_meter[0]) <= SUM_RTOL * ref_meter[0]
    assert got_m[0] == start[0] + got["loss"][0] * want.n_crops, "the meter takes the loss the call wrote, times the total crop count"
    again, _ = run_combine(parts, J, h, w)                       # no meter; two runs give the same bits
    for n in got:
        assert np.array_equal(got[n], again[n]), n


def test_bad_arguments_and_all_empty_parts():
    J, h, w = 5, 9, 7
    parts = draw_parts(np.random.default_rng(5), 4, J)
    m = guarded_meter([1.0, 2.0, 3.0, 4.0])
    mp = m.data_ptr() + 8 * GUARD
    for bad in (dict(n_part=0), dict(n_part=-1), dict(joints=0), dict(joints=-2), dict(h=0), dict(w=0), dict(h=-1), dict(parts=None), dict(sse=None),
                dict(hits=None), dict(valid=None), dict(loss=None), dict(acc=None), dict(avg_acc=None), dict(cnt=None), dict(n_crops=None)):
        _, o = run_combine(parts, J, h, w, meter=mp, expect=-1, bad=bad)
        assert all(g.untouched() for g in o.values()), bad
        assert b"i2r_val_combine" in cabi.lib().i2r_last_error()
    assert meter_of(m).tolist() == [1.0, 2.0, 3.0, 4.0]
    assert cabi.lib().i2r_val_combine(None, None) == -1
    # no crop anywhere: zeros everywhere (acc too, not -1), the meter left alone -- whatever the rows hold behind their count
    empty = parts.copy()
    empty[:, 0] = [0.0, -1.0, 0.0, -0.0]
    got, _ = run_combine(empty, J, h, w, meter=mp)
    for n, v in got.items():
        assert (v == 0).all() and not (v.dtype == np.float64 and np.signbit(v).any()), n
    assert meter_of(m).tolist() == [1.0, 2.0, 3.0, 4.0]
    got, _ = run_combine(np.zeros((1, 1 + 3 * J)), J, h, w, meter=mp)
    assert all((v == 0).all() for v in got.values()) and meter_of(m).tolist() == [1.0, 2.0, 3.0, 4.0]
    # the Python surface: the same, and n_crops is there
    vm = caller.ValMeter(dev())
    r = caller.val_combine(up(empty, np.float64), h, w, meter=vm)
    assert r.pred is None and r.n_crops.item() == 0 and r.acc.tolist() == [0.0] * (J + 1) and r.loss.item() == 0 and vm.buf.tolist() == [0.0] * 4


# ---- one part: i2r_val_metrics' own numbers, bit for bit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", [3, 2])
def test_one_part_reproduces_val_metrics_bit_for_bit(ci, monkeypatch):
    d = case(ci)
    assert (d.S, d.J, d.h, d.w) in ((3, 14, 17, 13), (5, 17, 20, 20))
    out, hm, vis = up(d.output, np.float32), up(d.joints_hm, np.float64), up(d.joints_vis, np.float32)
    jw = None if d.jw is None else d.jw.copy()
    m_own, m_cmb = caller.ValMeter(dev()), caller.ValMeter(dev())
    syncs = []
    for sl in (slice(0, d.S), slice(1, 3)):                       # two steps of different size into both meters
        own = caller.val_metrics(out[sl], joints_hm=hm[sl], joints_vis=vis[sl], joints_weight=jw, sigma=d.sigma, meter=m_own)
        n = out[sl].shape[0]
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
        monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
        row = caller.val_sums_row(own, n)
        got = caller.val_combine(row[None], d.h, d.w, meter=m_cmb)
        monkeypatch.undo()
        assert syncs == [], "val_sums_row and val_combine run without a host synchronisation"
        assert row.dtype == F64 and row.shape == (1 + 3 * d.J,) and row[0].item() == n
        for name in ("loss", "acc", "avg_acc", "sse"):
            assert np.array_equal(bits(getattr(got, name).cpu().numpy()), bits(getattr(own, name).cpu().numpy())), (ci, name)
        for name in ("cnt", "hits", "valid"):
            assert torch.equal(getattr(got, name), getattr(own, name)), (ci, name)
        assert got.n_crops.item() == n and got.pred is None and own.loss.item() > 0
        assert np.array_equal(bits(m_cmb.buf.cpu().numpy()), bits(m_own.buf.cpu().numpy())), "the meter, step by step"
    assert m_own.buf[1].item() == d.S + 2


# ---- the reference's output cut into shards, on the device -------------------------------------------------------------------------------

def device_rows(d, shards, analytic, use_w=True):
    """caller.val_metrics per shard (an empty one launches nothing and returns zeros), the rows stacked as the gather stacks them"""
    out = up(d.output, np.float32)
    rows, lo = [], 0
    for n in shards:
        sl = slice(lo, lo + n)
        if analytic:
            m = caller.val_metrics(out[sl], joints_hm=d.joints_hm[sl].copy(), joints_vis=d.joints_vis[sl].copy(), sigma=d.sigma,
                                   joints_weight=None if d.jw is None else d.jw.copy(), use_target_weight=use_w)
        else:
            m = caller.val_metrics(out[sl], up(d.target[sl], np.float32), up(d.target_weight[sl], np.float32), use_target_weight=use_w)
        rows.append(caller.val_sums_row(m, n))
        lo += n
    return torch.stack(rows)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("ci,shards", SHARDED)
def test_fixture_shards_combine_to_the_reference(ci, shards, analytic):
    d = case(ci)
    want = restated(ci, 1)           # (hits and valid: its acc / avg_acc / cnt equal the fixture's, tests/test_val_metrics.py)
    rows = device_rows(d, shards, analytic)
    assert rows.shape == (len(shards), 1 + 3 * d.J) and [int(v) for v in rows[:, 0].tolist()] == list(shards)
    got = caller.val_combine(rows, d.h, d.w)
    again = caller.val_combine(rows.clone(), d.h, d.w)
    assert got.n_crops.item() == d.S
    assert np.array_equal(bits(got.acc.cpu().numpy()), bits(d.acc)) and bits(got.avg_acc.cpu().numpy())[0] == bits(float(d.avg_acc))
    assert got.cnt.item() == int(d.cnt)
    assert np.array_equal(got.hits.cpu().numpy(), want.hits) and np.array_equal(got.valid.cpu().numpy(), want.valid)
    loss, loss64 = got.loss.item(), float(d.loss64_w1)
    if analytic:
        bound = analytic_loss_bound(d.output, d.target, d.target_weight, True)
        print("case %d shards %s analytic: loss %.17g, float64 %.17g, |diff| %.3g, bound %.3g" % (ci, shards, loss, want.loss, abs(loss - want.loss), bound))
        assert abs(loss - want.loss) <= bound
    else:
        print("case %d shards %s tensor: loss %.17g, fixture float64 %.17g, rel %.3g (bound %.3g)" % (ci, shards, loss, loss64, abs(loss - loss64) / loss64, SUM_RTOL))
        assert abs(loss - loss64) <= SUM_RTOL * loss64
        assert (np.abs(got.sse.cpu().numpy() - want.sse) <= SUM_RTOL * want.sse).all()
    for name in ("loss", "acc", "avg_acc", "sse", "cnt", "hits", "valid", "n_crops"):
        assert torch.equal(getattr(got, name), getattr(again, name)), name
    assert bits(got.loss.cpu().numpy())[0] == bits(again.loss.cpu().numpy())[0]


# ---- behind the model ----------------------------------------------------------------------------------------------------------------

def test_end_to_end_forward_flip_shards_equal_the_whole_batch():
    """tph_l21 through forward_flip; the heat maps cut by shard_bounds(length, 3) as three ranks would hold them; val_metrics per shard,
    combined, against val_metrics on the whole output.  The joints are those of tests/test_val_metrics_gpu.py's end-to-end test."""
    cfg, sd, x, m, length, g = setup("tph_l21")
    net = models.interformer.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    y = net.forward_flip(x.cuda(), m.cuda(), length, caller.FLIP_PAIRS["crowdpose"])
    S, J, h, w = y.shape
    peak = _val_ref.max_preds(g["out_multi"]).astype(np.float64)
    offsets = np.array([[0.25, -0.25], [0.0, 0.3], [1.25, 0.0], [-0.3, 2.2], [4.25, 3.75], [-60.0, 0.25], [0.3, 80.0]])
    mu = peak + offsets[(np.arange(S)[:, None] * 3 + np.arange(J)[None, :]) % len(offsets)]
    vis = np.ones((S, J), np.float32)
    vis[0, 3] = vis[2, 5] = 0
    whole_meter, all_meter = caller.ValMeter(y.device), caller.ValMeter(y.device)
    whole = caller.val_metrics_cfg(cfg, y, joints_hm=mu, joints_vis=vis, meter=whole_meter)
    b = i2r_dist.shard_bounds(length, 3)
    cuts = [sum(length[:i]) for i in b]
    assert len(b) == 4 and cuts[0] == 0 and cuts[-1] == S and cuts[1] > 0   # (fewer images than ranks: the trailing rank is empty)
    rows = []
    for lo, hi in zip(cuts, cuts[1:]):
        part = caller.val_metrics_cfg(cfg, y[lo:hi], joints_hm=mu[lo:hi], joints_vis=vis[lo:hi])
        rows.append(caller.val_sums_row(part, hi - lo))
    got = caller.val_combine(torch.stack(rows), h, w, meter=all_meter)
    assert 0 < whole.valid.sum().item() < S * J
    for name in ("acc", "avg_acc"):
        assert np.array_equal(bits(getattr(got, name).cpu().numpy()), bits(getattr(whole, name).cpu().numpy())), name
    for name in ("cnt", "hits", "valid"):
        assert torch.equal(getattr(got, name), getattr(whole, name)), name
    assert got.n_crops.item() == S
    a, ref = got.loss.item(), whole.loss.item()
    print("end to end: combined loss %.17g, whole-batch %.17g, rel %.3g (bound %.3g)" % (a, ref, abs(a - ref) / ref, SUM_RTOL))
    assert ref > 0 and abs(a - ref) <= SUM_RTOL * ref
    assert (torch.abs(got.sse - whole.sse) <= SUM_RTOL * whole.sse).all()
    am, wm = all_meter.buf.cpu().numpy(), whole_meter.buf.cpu().numpy()
    assert am[1] == wm[1] == S and am[3] == wm[3] and am[2] == wm[2] and abs(am[0] - wm[0]) <= SUM_RTOL * wm[0]


# ---- RCCL, one rank ------------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def nccl_world1():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_rccl_world1_val_metrics_all_equals_val_metrics(nccl_world1):
    d = case(2)
    out, hm, vis = up(d.output, np.float32), up(d.joints_hm, np.float64), up(d.joints_vis, np.float32)
    m_own, m_all = caller.ValMeter(dev()), caller.ValMeter(dev())
    for sl in (slice(0, 5), slice(2, 4)):
        own = caller.val_metrics(out[sl], joints_hm=hm[sl], joints_vis=vis[sl], joints_weight=d.jw.copy(), sigma=d.sigma, meter=m_own)
        n = out[sl].shape[0]
        rows = i2r_dist.gather_val_sums(own, n)
        assert rows.is_cuda and rows.shape == (1, 1 + 3 * d.J) and torch.equal(rows[0], caller.val_sums_row(own, n))
        got = i2r_dist.val_metrics_all(own, n, d.h, d.w, meter=m_all)
        for name in ("loss", "acc", "avg_acc", "sse"):
            assert np.array_equal(bits(getattr(got, name).cpu().numpy()), bits(getattr(own, name).cpu().numpy())), name
        for name in ("cnt", "hits", "valid"):
            assert torch.equal(getattr(got, name), getattr(own, name)), name
        assert got.n_crops.item() == n
        assert np.array_equal(bits(m_all.buf.cpu().numpy()), bits(m_own.buf.cpu().numpy()))
    assert m_all.result() == m_own.result() and m_all.result()[0] > 0


# ---- PoseTable -----------------------------------------------------------------------------------------------------------------------

def test_pose_table_evaluates_like_one_oks_eval_call(monkeypatch):
    """six images in three steps of two emulated ranks (one image each; the rows of a step stacked in rank order as gather_poses does),
    appended across two growth boundaries; an image without detections and a suppressed row are among them"""
    J = 17
    rng = np.random.default_rng(31)
    sizes = [(4, 2), (0, 2), (6, 3), (3, 0), (5, 4), (7, 2)]       # (detections, persons) per image
    per = [draw_image(rng, i + 1, nd, ng, J, caller.SIGMAS[J])[:2] for i, (nd, ng) in enumerate(sizes)]
    ids = list(range(1, len(sizes) + 1))
    gt = caller.GtTable.from_coco(coco_dict([g for gs, _ in per for g in gs], ids))
    blocks = []                                                    # per image: (rows [n, J * 3 + 2] on the device, image ids)
    for img, (_, dts) in zip(ids, per):
        kp = np.asarray([d["keypoints"] for d in dts], np.float32).reshape(len(dts), J * 3)
        sc = np.asarray([d["score"] for d in dts], np.float32).reshape(len(dts), 1)
        rank = np.arange(len(dts), dtype=np.float32).reshape(len(dts), 1)
        if img == 3:
            rank[1] = -1.0                                         # suppressed by the NMS of its rank
        blocks.append((torch.from_numpy(np.concatenate([kp, sc, rank], 1)).to(dev()), [img] * len(dts)))
    table = caller.PoseTable(J, dev(), capacity=4)
    syncs = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    for step in range(3):
        (r0, i0), (r1, i1) = blocks[2 * step], blocks[2 * step + 1]
        table.append(torch.cat([r0, r1]), i0 + i1)
    monkeypatch.undo()
    assert syncs == [], "append makes no host synchronisation"
    rows = torch.cat([b for b, _ in blocks])
    all_ids = [i for _, l in blocks for i in l]
    assert len(table) == 25 and table.buf.shape[0] == 32 and torch.equal(table.rows(), rows) and table.image_ids().tolist() == all_ids
    kp, score, rank = i2r_dist.unpack_poses(rows)
    assert (rank < 0).sum().item() == 1 and 2 not in all_ids
    want = caller.oks_eval(gt, all_ids, kp, score, rank >= 0)
    got = table.evaluate(gt)
    for name in ("stats", "precision", "recall", "npig"):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert (want.precision[0, :, :, 0] > 0).any() and (want.npig[0] > 0).any()
    unmasked = caller.oks_eval(gt, all_ids, kp, score)
    assert not torch.equal(unmasked.match["rank"], want.match["rank"]), "the suppressed row is masked out, not evaluated"
