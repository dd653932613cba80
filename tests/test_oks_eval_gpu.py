"""-m gpu: i2r_oks_match and i2r_oks_accumulate through the raw C-ABI (canaries of 64 elements around every output) and caller.oks_eval end
to end, against the float64 restatement tests/_cocoeval_ref.py.  Inputs come from the seeded generator of tests/_oks_cases.py: every
image is redrawn on the CPU until every comparison the restatement makes lies >= 1e-9 from a tie, so that the discrete outcome does not
depend on the last ulp of exp(); the achieved minimum is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import _cocoeval_ref as ref
from i2r_amd import cabi, caller
from _oks_cases import HAND, MARGIN, SIGMAS14, coco_dict, draw_image, walk_margins

pytestmark = pytest.mark.gpu

GUARD = 64
C_RANK, C_BITS, C_U8, C_F64 = -77, 0x5A5A5A5A, 0xA5, -12345.5
SIZES = [(0, 0), (0, 3), (3, 0), (1, 1), (5, 4), (20, 7), (21, 7), (40, 33), (300, 200)]   # (detections, gts) of one image
THR, REC, AREA = caller.OKS_THRS, caller.OKS_REC_THRS, caller.OKS_AREA_RNG
DEV = "cuda"


def _guarded(n, dtype, fill):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)


def _strip(t, fill):
    a = t.cpu().numpy()
    assert (a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all(), "canary overwritten"
    return a[GUARD:-GUARD]


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(DEV)


class Set:
    """per-image (gts, dts) lists -> the tables of i2r_oks_match on the device, outputs with canaries; run() is the raw call on a range
    of images"""

    def __init__(self, per_image, J, sigmas, valid=None):
        self.J, self.per = J, per_image
        self.gts = [g for gs, _ in per_image for g in gs]
        self.dts = [d for _, ds in per_image for d in ds]
        self.n_img, self.n_gt, self.n_dt = len(per_image), len(self.gts), len(self.dts)
        self.ids = [i + 1 for i in range(self.n_img)]
        self.gcount = np.asarray([len(gs) for gs, _ in per_image], np.int64)
        self.dcount = np.asarray([len(ds) for _, ds in per_image], np.int64)
        self.goff = np.concatenate([[0], np.cumsum(self.gcount)]).astype(np.int32)
        self.doff = np.concatenate([[0], np.cumsum(self.dcount)]).astype(np.int32)
        self.ooff = np.concatenate([[0], np.cumsum(self.gcount * self.dcount)]).astype(np.int64)
        gk = np.asarray([g["keypoints"] for g in self.gts], np.float64).reshape(self.n_gt, J, 3)
        dk = np.asarray([d["keypoints"] for d in self.dts], np.float64).reshape(self.n_dt, J, 3)[:, :, :2]
        assert np.array_equal(dk.astype(np.float32).astype(np.float64), dk), "the detections are exact in fp32"
        self.sigmas = sigmas
        self.valid = None if valid is None else np.asarray(valid, bool)
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)
        self.t = dict(dt_kpts=torch.from_numpy(dk.astype(np.float32)).to(DEV),
                      dt_score=torch.from_numpy(np.asarray([d["score"] for d in self.dts], np.float32)).to(DEV),
                      dt_valid=None if valid is None else torch.from_numpy(self.valid.astype(np.uint8)).to(DEV),
                      dt_off=i32(self.doff), gt_kpts=_f64(gk), gt_area=_f64([g["area"] for g in self.gts]),
                      gt_bbox=_f64(np.asarray([g["bbox"] for g in self.gts]).reshape(self.n_gt, 4)),
                      gt_flags=i32([int(bool(g["iscrowd"])) | (int(bool(g["iscrowd"]) or g["num_keypoints"] == 0) << 1) for g in self.gts]),
                      gt_off=i32(self.goff), sigmas=_f64(sigmas), thr=_f64(THR), area_rng=_f64(AREA),
                      oks_off=torch.from_numpy(self.ooff).to(DEV))
        self.reset()

    def reset(self):
        nA = len(AREA)
        self.rank = _guarded(self.n_dt, torch.int32, C_RANK)
        self.match = _guarded(nA * self.n_dt, torch.int32, C_BITS)
        self.ignore = _guarded(nA * self.n_dt, torch.int32, C_BITS)
        self.gti = _guarded(nA * self.n_gt, torch.uint8, C_U8)
        self.oks = _guarded(int(self.ooff[-1]), torch.float64, C_F64)

    def run(self, img_lo=0, img_hi=None, expect=0, want_oks=True, **kw):
        img_hi = self.n_img if img_hi is None else img_hi
        t = self.t
        p = lambda x: None if x is None else x.data_ptr()
        a = cabi.OksMatchArgs(dt_kpts=p(t["dt_kpts"]), dt_score=p(t["dt_score"]), dt_valid=p(t["dt_valid"]), dt_off=p(t["dt_off"]) + 4 * img_lo,
                              gt_kpts=p(t["gt_kpts"]), gt_area=p(t["gt_area"]), gt_bbox=p(t["gt_bbox"]), gt_flags=p(t["gt_flags"]),
                              gt_off=p(t["gt_off"]) + 4 * img_lo, sigmas=p(t["sigmas"]), thr=p(t["thr"]), area_rng=p(t["area_rng"]),
                              dt_rank=self.rank.data_ptr() + 4 * GUARD, dt_match=self.match.data_ptr() + 4 * GUARD,
                              dt_ignore=self.ignore.data_ptr() + 4 * GUARD, gt_ignore=self.gti.data_ptr() + GUARD,
                              oks=self.oks.data_ptr() + 8 * GUARD if want_oks else None, oks_off=p(t["oks_off"]) + 8 * img_lo,
                              oks_len=int(self.ooff[-1]), n_dt=self.n_dt, n_gt=self.n_gt, n_img=img_hi - img_lo, joints=self.J, n_thr=len(THR),
                              n_area=len(AREA), max_dets=20, max_dt_per_img=int(max(self.dcount[img_lo:img_hi].tolist() + [0])),
                              max_gt_per_img=int(max(self.gcount[img_lo:img_hi].tolist() + [0])))
        for k, v in kw.items():
            setattr(a, k, v)
        rc = cabi.lib().i2r_oks_match(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, cabi.lib().i2r_last_error())
        torch.cuda.synchronize()
        return self

    def outputs(self):
        nA = len(AREA)
        return (_strip(self.rank, C_RANK), _strip(self.match, C_BITS).view(np.uint32).reshape(nA, self.n_dt),
                _strip(self.ignore, C_BITS).view(np.uint32).reshape(nA, self.n_dt), _strip(self.gti, C_U8).reshape(nA, self.n_gt),
                _strip(self.oks, C_F64))

    def untouched(self):
        r, m, i, g, o = self.outputs()
        return (r == C_RANK).all() and (m == C_BITS).all() and (i == C_BITS).all() and (g == C_U8).all() and (o == C_F64).all()

    def expected(self, img_lo=0, img_hi=None, max_dets=20):
        """the restatement on the detections that exist, as the arrays of the C-ABI; where the kernel writes nothing: the canary value.
        -> (rank, match, ignore, gt_ignore, oks, the smallest margin of the restatement's comparisons)"""
        img_hi = self.n_img if img_hi is None else img_hi
        nA, T = len(AREA), len(THR)
        rank = np.full(self.n_dt, C_RANK, np.int32)
        match = np.full((nA, self.n_dt), C_BITS, np.uint32)
        ign = np.full((nA, self.n_dt), C_BITS, np.uint32)
        gti = np.full((nA, self.n_gt), C_U8, np.uint8)
        oks = np.full(int(self.ooff[-1]), C_F64, np.float64)
        d0, d1, g0, g1 = self.doff[img_lo], self.doff[img_hi], self.goff[img_lo], self.goff[img_hi]
        rank[d0:d1], match[:, d0:d1], ign[:, d0:d1] = -1, 0, 0
        oks[self.ooff[img_lo]:self.ooff[img_hi]] = -1.0
        keep = [k for k in range(d0, d1) if self.valid is None or self.valid[k]]
        gts = self.gts[g0:g1]
        if max_dets == 20:
            e = ref.run(gts, [self.dts[k] for k in keep], self.ids[img_lo:img_hi], self.sigmas)
        else:   # (another Params.maxDets: evaluate() alone, summarize's table is about 20)
            e = ref.CocoEvalRef(gts, [self.dts[k] for k in keep], self.ids[img_lo:img_hi], self.sigmas)
            e.params.maxDets = [max_dets]
            e.evaluate()
        margins = walk_margins(e)
        n = img_hi - img_lo
        bits = lambda col: int(sum(1 << t for t in range(T) if col[t]))
        for a in range(nA):
            for i in range(n):
                E = e.evalImgs[a * n + i]
                if E is None:
                    continue
                for r, did in enumerate(E["dtIds"]):
                    k = keep[did - 1]
                    rank[k] = r
                    match[a, k], ign[a, k] = bits(E["dtMatches"][:, r] != 0), bits(E["dtIgnore"][:, r])
                    if a == 0 and len(e.ious[E["image_id"]]):
                        img = img_lo + i
                        G = int(self.gcount[img])
                        at = int(self.ooff[img]) + (k - int(self.doff[img])) * G
                        oks[at:at + G] = e.ious[E["image_id"]][r]
                for j, gid in enumerate(E["gtIds"]):
                    gti[a, g0 + gid - 1] = E["gtIgnore"][j]
        return rank, match, ign, gti, oks, (min(margins) if margins else 1.0)


def _draw_set(seed, J, sigmas, sizes, **kw):
    rng = np.random.default_rng(seed)
    per, low = [], 1.0
    for i, (nd, ng) in enumerate(sizes):
        g, d, m = draw_image(rng, i + 1, nd, ng, J, sigmas, **kw)
        per.append((g, d))
        low = min(low, m)
    assert low >= MARGIN
    return per, rng


def _check(s, want, what):
    rank, match, ign, gti, oks = s.outputs()
    w_rank, w_match, w_ign, w_gti, w_oks, low = want
    print(what, "smallest margin %.3e, largest OKS error %.3e" % (low, np.abs(oks - w_oks).max() if oks.size else 0.0))
    assert low >= MARGIN, "an input property: the restatement's own comparisons are not on a tie"
    assert np.array_equal(rank, w_rank), what
    assert np.array_equal(gti, w_gti), what
    assert np.array_equal(match, w_match) and np.array_equal(ign, w_ign), what
    assert (np.abs(oks - w_oks) <= 1e-12).all(), what


@pytest.mark.parametrize("J", [17, 14])
def test_match_sizes(J):
    """every (detections, gts) size in one launch, with and without a dt_valid mask that removes a third; then a sub-range of images"""
    sigmas = caller.SIGMAS[17] if J == 17 else SIGMAS14   # (J = 14: a second table)
    per, rng = _draw_set(100 + J, J, sigmas, SIZES)
    s = Set(per, J, sigmas)
    assert any(g["iscrowd"] for g in s.gts) and any(g["num_keypoints"] == 0 for g in s.gts)
    assert {32.0 ** 2, 96.0 ** 2} <= set(g["area"] for g in s.gts), "areas exactly on the bounds"
    assert len(set(d["score"] for d in s.dts)) < s.n_dt, "score ties"
    want = s.expected()
    _check(s.run(), want, "all")
    assert (want[0] >= 0).sum() == sum(min(nd, 20) for nd, _ in SIZES) and (want[3] == 1).any() and (want[1] != 0).any()
    for attempt in range(20):   # a mask under which the restatement's comparisons keep their margin
        masked = Set(per, J, sigmas, valid=rng.uniform(size=s.n_dt) < 2.0 / 3.0)
        want = masked.expected()
        if want[5] >= MARGIN:
            break
    assert not masked.valid.all()
    _check(masked.run(), want, "masked")
    masked.reset()
    _check(masked.run(4, 7), masked.expected(4, 7), "images 4 ... 6")
    masked.reset()
    _check(masked.run(8, 9, want_oks=False), masked.expected(8, 9)[:4] + (np.full_like(want[4], C_F64), want[5]), "the largest image, no oks")


def test_match_at_the_limits_32_detections_250_gts():
    """max_dets = 32 on an image of 40 detections and 250 gts: the largest OKS matrix in LDS (32 x 250 x 8 bytes, the raised limit)"""
    J, sigmas = 17, caller.SIGMAS[17]
    for seed in range(300, 310):   # a draw whose comparisons keep their margin with 32 detections in the walk too
        # (plain gts: among 250 on one canvas the widened boxes of gts without labelled points overlap, and a detection inside two of
        # them has OKS exactly 1 with both; crowd, bbox and area cases are test_match_sizes')
        per, _ = _draw_set(seed, J, sigmas, [(3, 2), (40, 250), (1, 1)], special=False)
        s = Set(per, J, sigmas)
        want = s.expected(max_dets=32)
        if want[5] >= MARGIN:
            break
    assert (want[0] >= 0).sum() == 3 + 32 + 1 and want[0].max() == 31
    _check(s.run(max_dets=32), want, "max_dets 32")


def test_match_refused_bounds_write_nothing():
    per, _ = _draw_set(7, 17, caller.SIGMAS[17], [(5, 4), (3, 2)])
    s = Set(per, 17, caller.SIGMAS[17])
    for bad in (dict(max_dets=33), dict(max_gt_per_img=257), dict(max_dt_per_img=1025), dict(joints=33), dict(joints=0), dict(n_thr=17),
                dict(n_area=5)):
        s.run(expect=-1, **bad)
        assert s.untouched(), bad
    s.run(n_img=0)
    assert s.untouched(), "no image: no launch"
    # an image that holds more than the host-side bound it was launched with: -1 ranks for its own detections, nothing else
    s.run(max_dt_per_img=4)
    rank, match, ign, gti, oks = s.outputs()
    want = s.expected(1, 2)
    assert (rank[:5] == -1).all() and np.array_equal(rank[5:], want[0][5:])
    assert (match[:, :5] == C_BITS).all() and (ign[:, :5] == C_BITS).all() and (gti[:, :4] == C_U8).all() and (oks[:20] == C_F64).all()
    assert np.array_equal(match[:, 5:], want[1][:, 5:]) and np.array_equal(gti[:, 4:], want[3][:, 4:])


# ---- accumulate ----------------------------------------------------------------------------------------------------------------------
def _accumulate_case(n_part, seed, nT, nA, n_group, n_img=40):
    """flags drawn directly: -> the argument tables (numpy) and the restatement's precision / recall / npig"""
    rng = np.random.default_rng(seed)
    n_gt = 3 * n_img
    gt_img = np.sort(rng.integers(0, n_img, n_gt))
    gt_off = np.searchsorted(gt_img, np.arange(n_img + 1)).astype(np.int32)
    gti = (rng.uniform(size=(nA, n_gt)) < .3).astype(np.uint8)
    gti[nA - 1] = 1                                                   # an area range without a counted gt: npig == 0
    img_group = rng.integers(-1, max(n_group - 1, 0), n_img).astype(np.int32)   # the last group holds no image
    dt_img = np.sort(rng.integers(0, n_img, n_part)).astype(np.int32)
    score = (rng.integers(0, max(n_part // 3, 2), n_part) / 2.0 ** 20).astype(np.float32)   # ties, inside and across images
    rank = np.where(rng.uniform(size=n_part) < .05, -1, 0).astype(np.int32)        # some take no part
    order = np.argsort(-score.astype(np.float64), kind="mergesort").astype(np.int32)
    match = rng.integers(0, 1 << nT, (nA, n_part)).astype(np.uint32)
    ign = (rng.integers(0, 1 << nT, (nA, n_part)) & rng.integers(0, 1 << nT, (nA, n_part))).astype(np.uint32)
    rec = np.asarray(REC)
    prec = -np.ones((n_group + 1, nT, len(rec), nA))
    recall = -np.ones((n_group + 1, nT, nA))
    npig = np.zeros((n_group + 1, nA), np.int32)
    part = order[rank[order] >= 0]
    for g in range(n_group + 1):
        in_img = np.ones(n_img, bool) if g == n_group else img_group == g
        sel = part[in_img[dt_img[part]]]
        for a in range(nA):
            npig[g, a] = int(sum((gti[a, gt_off[i]:gt_off[i + 1]] == 0).sum() for i in range(n_img) if in_img[i]))
            if npig[g, a] == 0:
                continue
            dtm = np.stack([(match[a, sel] >> t) & 1 for t in range(nT)]).astype(bool).reshape(nT, len(sel))
            dti = np.stack([(ign[a, sel] >> t) & 1 for t in range(nT)]).astype(bool).reshape(nT, len(sel))
            tps = np.logical_and(dtm, np.logical_not(dti))
            fps = np.logical_and(np.logical_not(dtm), np.logical_not(dti))
            prec[g, :, :, a], recall[g, :, a] = ref.accumulate_flags(tps, fps, npig[g, a], rec)
    return dict(gt_off=gt_off, gti=gti, img_group=img_group, dt_img=dt_img, rank=rank, order=order, match=match, ign=ign, n_gt=n_gt,
                n_img=n_img), prec, recall, npig


@pytest.mark.parametrize("n_part", [0, 1, 63, 64, 65, 1000, 1023, 1024, 1025, 70000])
def test_accumulate_sizes(n_part):
    """precision, recall and npig bit-identical to the restatement's accumulate on the same flags, twice; chunk boundaries (the kernel
    walks chunks of 1024) and many-chunk carries"""
    nT, nA, n_group = (2, 2, 1) if n_part > 2000 else (10, 3, 4)
    c, w_prec, w_rec, w_npig = _accumulate_case(n_part, 1000 + n_part, nT, nA, n_group)
    assert (w_npig[:, nA - 1] == 0).all() and (w_npig[n_group - 1] == 0).all() and (w_npig[n_group, 0] > 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = {k: up(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in c.items() if isinstance(v, np.ndarray)}
    rec = _f64(REC)
    R = len(REC)
    runs = []
    for _ in range(2):
        prec = _guarded((n_group + 1) * nT * R * nA, torch.float64, C_F64)
        recall = _guarded((n_group + 1) * nT * nA, torch.float64, C_F64)
        npig = _guarded((n_group + 1) * nA, torch.int32, C_RANK)
        p = lambda x: x.data_ptr() if x.numel() else None
        a = cabi.OksAccumulateArgs(dt_match=p(t["match"]), dt_ignore=p(t["ign"]), dt_rank=p(t["rank"]), order=p(t["order"]), dt_img=p(t["dt_img"]),
                                   img_group=p(t["img_group"]), gt_ignore=p(t["gti"]), gt_off=p(t["gt_off"]), rec_thr=rec.data_ptr(),
                                   precision=prec.data_ptr() + 8 * GUARD, recall=recall.data_ptr() + 8 * GUARD, npig=npig.data_ptr() + 4 * GUARD,
                                   n_dt=n_part, n_gt=c["n_gt"], n_img=c["n_img"], n_part=n_part, n_group=n_group, n_thr=nT, n_area=nA, n_rec=R)
        rc = cabi.lib().i2r_oks_accumulate(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, cabi.lib().i2r_last_error()
        torch.cuda.synchronize()
        runs.append((_strip(prec, C_F64).copy(), _strip(recall, C_F64).copy(), _strip(npig, C_RANK).copy()))
    b = lambda x: np.ascontiguousarray(x, np.float64).reshape(-1).view(np.int64)
    assert np.array_equal(runs[0][2], w_npig.reshape(-1))
    assert np.array_equal(b(runs[0][1]), b(w_rec)), "recall, bit for bit"
    assert np.array_equal(b(runs[0][0]), b(w_prec)), "precision, bit for bit"
    assert all(np.array_equal(b(x), b(y)) for x, y in zip(runs[0][:2], runs[1][:2])), "two runs, the same bits"
    if n_part >= 63:
        assert (w_prec[n_group, :, :, 0] > 0).any() and (w_rec[n_group, :, 0] > 0).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _eval(per, ids, J=17, perm=None, groups=None, **kw):
    gts = [g for gs, _ in per for g in gs]
    dts = [d for _, ds in per for d in ds]
    if perm is not None:
        dts = [dts[i] for i in perm]
    gt = caller.GtTable.from_coco(coco_dict(gts, ids))
    kp = torch.from_numpy(np.asarray([d["keypoints"] for d in dts], np.float32).reshape(len(dts), J, 3)).to(DEV)
    sc = torch.tensor([d["score"] for d in dts], dtype=torch.float32, device=DEV)
    return gt, gts, dts, caller.oks_eval(gt, [d["image_id"] for d in dts], kp, sc, groups=groups, **kw)


def test_end_to_end_with_person_count_groups():
    """200 images, the per-person-count table: the restatement on the whole set and, per level, on the images of that level alone"""
    rng = np.random.default_rng(11)
    n_gts = rng.choice([0, 1, 1, 2, 3, 4, 6, 8, 11, 14], 200)
    sizes = [(int(max(0, g + rng.integers(-1, 5))), int(g)) for g in n_gts]
    per, _ = _draw_set(12, 17, caller.SIGMAS[17], sizes)
    ids = list(range(1, 201))
    gt0 = caller.GtTable.from_coco(coco_dict([g for gs, _ in per for g in gs], ids), device="cpu")
    grp, names = caller.person_count_groups(gt0.counts)
    assert names == ["c1", "c2", "c3", "c4"] and set(grp.tolist()) == {-1, 0, 1, 2, 3}
    gt, gts, dts, ev = _eval(per, ids, groups=(grp, names))
    assert 1200 <= len(dts) <= 2000 and ev.group_names == ("c1", "c2", "c3", "c4", "all")
    stats = ev.stats.cpu().numpy()
    whole = ref.run(gts, dts, ids)
    print("all", stats[4].tolist(), "error %.3e" % np.abs(stats[4] - whole.stats).max())
    assert np.abs(stats[4] - whole.stats).max() <= 1e-12 and (whole.stats[[0, 5]] > 0.05).all()
    assert np.array_equal(ev.precision[4].cpu().numpy(), whole.eval["precision"][:, :, 0, :, 0]), "bit for bit, as accumulate's inputs are integers"
    assert np.array_equal(ev.npig[4].cpu().numpy(), whole.eval["npig"])
    for g, name in enumerate(names):
        sub = ref.run_subset(gts, dts, ids, [i for i, k in zip(ids, grp.tolist()) if k == g])
        print(name, stats[g].tolist(), "error %.3e" % np.abs(stats[g] - sub.stats).max())
        assert np.abs(stats[g] - sub.stats).max() <= 1e-12, name
        assert list(ev.name_values(name).items()) == list(zip(ref.STATS_NAMES, stats[g].tolist()))
    assert list(ev.name_values().values()) == stats[4].tolist()


def test_shuffled_detections_give_the_same_result():
    rng = np.random.default_rng(21)
    sizes = [(int(rng.integers(0, 26)), int(rng.integers(0, 6))) for _ in range(40)]
    per, _ = _draw_set(22, 17, caller.SIGMAS[17], sizes, distinct_scores=True)
    ids = list(range(1, 41))
    _, gts, dts, ev = _eval(per, ids)
    assert len(set(d["score"] for d in dts)) == len(dts), "a shuffle breaks no tie"
    _, _, _, ev2 = _eval(per, ids, perm=rng.permutation(len(dts)))
    assert torch.equal(ev.stats, ev2.stats) and torch.equal(ev.precision, ev2.precision) and torch.equal(ev.recall, ev2.recall)
    assert np.abs(ev.stats.cpu().numpy()[0] - ref.run(gts, dts, ids).stats).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived_cases_on_the_device(name):
    gts, dts, ids, want = HAND[name]
    gt = caller.GtTable.from_coco(coco_dict(gts, ids))
    kp = torch.tensor([d["keypoints"] for d in dts], dtype=torch.float32, device=DEV).reshape(len(dts), 17, 3)
    ev = caller.oks_eval(gt, [d["image_id"] for d in dts], kp, torch.tensor([d["score"] for d in dts], device=DEV))
    got = ev.stats.cpu().numpy()[0]
    assert np.abs(got - np.asarray([float(w) for w in want])).max() <= 1e-12, (name, got.tolist())


def test_valid_mask_and_three_column_key_points():
    """valid= removes detections as if they were not there (PoseNms.rank >= 0); [N, J, 3] key points: the third column is not read"""
    gts, dts, ids, _ = HAND["cut_at_20"]
    gt = caller.GtTable.from_coco(coco_dict(gts, ids))
    kp = torch.tensor([d["keypoints"] for d in dts], dtype=torch.float32, device=DEV).reshape(len(dts), 17, 3)
    sc = torch.tensor([d["score"] for d in dts], device=DEV)
    valid = torch.ones(len(dts), dtype=torch.bool, device=DEV)
    valid[5] = False   # one false positive less: the true positive is the 20th and is seen: AP = AR' = 1 / 20
    ev = caller.oks_eval(gt, [1] * len(dts), kp[:, :, :2], sc, valid)
    want = [0.05, 0.05, 0.05, 0.05, -1, 1, 1, 1, 1, -1]
    assert np.abs(ev.stats.cpu().numpy()[0] - np.asarray(want)).max() <= 1e-12
    assert ev.match["rank"].cpu().tolist().count(-1) == 1


# ---- behind the model ----------------------------------------------------------------------------------------------------------------
def test_behind_the_model_forward_decode_nms_eval(monkeypatch):
    """forward -> decode -> rescore_nms -> oks_eval against a ground truth built from the CPU oracle's own decoded poses: AP = AR = 1 in
    the populated area classes; then the poses shifted by a known OKS: the AP drops to the hand-computed step"""
    import i2r_cpu
    import post_cpu
    from _golden import setup
    from i2r_amd import models
    cfg, sd, x, m, length, g = setup("w48_l31")
    J = cfg.MODEL.NUM_JOINTS
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    S = int(sum(length))
    center = np.asarray([[300.0 + 700.0 * s, 400.0] for s in range(S)], np.float32)
    scale = np.asarray([[1.2, 1.6]] * S, np.float32)
    y = net.cuda()(x.cuda(), m.cuda(), length)
    preds, maxvals = caller.decode(y, center, scale, cfg.TEST.BLUR_KERNEL)
    nms = caller.rescore_nms_cfg(cfg, preds, maxvals, scale, torch.ones(S), length)
    ref_p, _ = post_cpu.get_final_preds(g["out_multi"], center, scale, cfg.TEST.BLUR_KERNEL)
    img_of = [i for i, n in enumerate(length) for _ in range(int(n))]
    area = 150.0 ** 2                                            # 'large'
    kp3 = np.concatenate([ref_p.astype(np.float64), np.full((S, J, 1), 2.0)], 2)
    lo, hi = ref_p.min(1), ref_p.max(1)
    gt = caller.GtTable.from_arrays(list(range(len(length))), img_of, kp3, [area] * S, np.concatenate([lo, hi - lo], 1))
    caller.oks_eval_cfg(cfg, gt, img_of, preds, nms.score, nms.rank >= 0)   # (the first call uploads the constant tables, once per device)
    syncs = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    ev = caller.oks_eval_cfg(cfg, gt, img_of, preds, nms.score, nms.rank >= 0, groups=caller.person_count_groups(gt.counts))
    assert syncs == [], "oks_eval runs without a host synchronisation or a copy to the host"
    named = ev.name_values()
    assert syncs == ["cpu"], "name_values() is the one copy to the host"
    monkeypatch.undo()
    stats = ev.stats.cpu().numpy()[-1]
    assert list(named.values()) == stats.tolist() and list(named) == ref.STATS_NAMES
    print("decode against the oracle's: %.3e px" % np.abs(preds.cpu().numpy() - ref_p).max(), stats.tolist())
    assert (nms.rank >= 0).all().item()
    assert np.abs(stats - np.asarray([1, 1, 1, -1, 1, 1, 1, 1, -1, 1.0])).max() <= 1e-12
    # every point shifted by d px in x: e_j = d^2 / (2 sigma_j)^2 / area / 2, OKS = mean_j exp(-e_j) (+ the decode difference, ~1e-3 px)
    sig = np.asarray(caller.SIGMAS[J])
    oks_of = lambda d: float(np.mean(np.exp(-d * d / (2 * sig) ** 2 / area / 2)))
    d = 30.0
    while not 0.62 < oks_of(d) < 0.63:   # between the thresholds .6 and .65
        d *= 1.005 if oks_of(d) > 0.625 else 0.995
    shifted = preds + torch.tensor([d, 0.0], device=DEV)
    ev = caller.oks_eval_cfg(cfg, gt, img_of, shifted, nms.score, nms.rank >= 0)
    # matched at the thresholds .5, .55, .6 (3 of 10) and unmatched above: AP = AR = 3 / 10, AP .5 = 1, AP .75 = 0
    want = [0.3, 1, 0, -1, 0.3, 0.3, 1, 0, -1, 0.3]
    assert np.abs(ev.stats.cpu().numpy()[0] - np.asarray(want)).max() <= 1e-12, (oks_of(d), ev.stats.cpu().tolist())
