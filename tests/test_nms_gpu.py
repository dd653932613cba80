"""-m gpu: i2r_pose_nms (rescoring + OKS-NMS / soft-OKS-NMS on the device) against the reference's own output
(tests/golden/nms_reference.npz: rank and n_keep identical, score bit-identical), against the float64 restatement tests/_nms_ref.py for
inputs the fixture does not hold, and end to end behind the model, caller.decode and dist.PostStep."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist

import _nms_ref
from _golden import setup
from i2r_amd import cabi, caller, config, models
from i2r_amd import dist as i2r_dist
from test_nms import JOINTS, combos, fixture, image_set, ranks_of

pytestmark = pytest.mark.gpu

GUARD = 64                               # canary elements on either side of every output
C_SCORE, C_RANK, C_KEEP = -12345.5, -77, -99


class Raw:
    """One set's inputs on the device + outputs with canaries around them; run() is the raw C-ABI call on a range of images."""

    def __init__(self, preds, maxvals, box_score, length, sigmas, area=None, scale=None):
        dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
        self.S, self.J = preds.shape[0], preds.shape[1]
        self.length = [int(v) for v in length]
        self.preds, self.maxvals, self.box, self.sig = up(preds), up(maxvals), up(box_score), up(sigmas)
        self.area = up(area) if area is not None else None
        self.scale = up(scale) if scale is not None else None
        self.prefix = np.concatenate([[0], np.cumsum(self.length)]).astype(np.int32)
        self.off = torch.from_numpy(self.prefix).to(dev)
        self.reset()

    def reset(self):
        dev, n_img = self.preds.device, len(self.length)
        self.score = torch.full((self.S + 2 * GUARD,), C_SCORE, dtype=torch.float32, device=dev)
        self.rank = torch.full((self.S + 2 * GUARD,), C_RANK, dtype=torch.int32, device=dev)
        self.n_keep = torch.full((n_img + 2 * GUARD,), C_KEEP, dtype=torch.int32, device=dev)

    def run(self, in_vis_thre, oks_thre, soft, img_lo=0, img_hi=None, oks_vis_thre=None, max_persons=None, expect=0, use_scale=False, **kw):
        img_hi = len(self.length) if img_hi is None else img_hi
        bound = max(self.length[img_lo:img_hi] + [1]) if max_persons is None else max_persons
        a = cabi.PoseNmsArgs(preds=self.preds.data_ptr(), maxvals=self.maxvals.data_ptr(),
                             scale=self.scale.data_ptr() if use_scale else None, area=None if use_scale else self.area.data_ptr(),
                             box_score=self.box.data_ptr(), img_off=self.off.data_ptr() + 4 * img_lo, sigmas=self.sig.data_ptr(),
                             score=self.score.data_ptr() + 4 * GUARD, rank=self.rank.data_ptr() + 4 * GUARD,
                             n_keep=self.n_keep.data_ptr() + 4 * (GUARD + img_lo), in_vis_thre=in_vis_thre, oks_thre=oks_thre,
                             oks_vis_thre=oks_vis_thre or 0.0, n_crops=self.S, n_img=img_hi - img_lo, joints=self.J, max_persons=bound,
                             soft=int(soft), max_dets=20, use_oks_vis=int(oks_vis_thre is not None))
        for k, v in kw.items():
            setattr(a, k, v)
        rc = cabi.lib().i2r_pose_nms(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
        assert rc == expect, (rc, cabi.lib().i2r_last_error())
        torch.cuda.synchronize()
        return self

    def outputs(self):
        """-> (score, rank, n_keep) numpy, canaries stripped AFTER checking them"""
        s, r, k = self.score.cpu().numpy(), self.rank.cpu().numpy(), self.n_keep.cpu().numpy()
        for a, c in ((s, np.float32(C_SCORE)), (r, C_RANK), (k, C_KEEP)):
            assert (a[:GUARD] == c).all() and (a[-GUARD:] == c).all(), "canary overwritten"
        return s[GUARD:-GUARD], r[GUARD:-GUARD], k[GUARD:-GUARD]


def _raw_of(d, **kw):
    return Raw(d["preds"], d["maxvals"], d["box_score"], d["length"], d["sigmas"], area=d["area"], scale=d["scale"], **kw)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("J", JOINTS)
def test_every_fixture_image_equals_the_reference(J, soft):
    """one launch per image: rank and n_keep identical to the reference's keep list, score bit-identical; nothing outside the image's
    own crops / own n_keep slot is written (the rest of the buffers keeps its canary value)"""
    f = fixture()
    for thr, vis in combos(f):
        d = image_set(f, J, thr, vis)
        keep = d["keep_soft" if soft else "keep_hard"]
        want_rank = ranks_of(keep, d["length"])
        want_score = d["score"].astype(np.float32)
        raw = _raw_of(d)
        for i, n in enumerate(d["length"]):
            raw.reset()
            score, rank, n_keep = raw.run(vis, thr, soft, i, i + 1, use_scale=bool(i & 1)).outputs()
            lo, hi = int(raw.prefix[i]), int(raw.prefix[i + 1])
            assert n_keep[i] == len(keep[i]), (J, thr, vis, i, n_keep[i], len(keep[i]))
            assert np.array_equal(rank[lo:hi], want_rank[lo:hi]), (J, thr, vis, i)
            assert np.array_equal(_bits(score[lo:hi]), _bits(want_score[lo:hi])), (J, thr, vis, i)
            inside = np.zeros(raw.S, bool)
            inside[lo:hi] = True
            assert (score[~inside] == np.float32(C_SCORE)).all() and (rank[~inside] == C_RANK).all()
            assert (np.delete(n_keep, i) == C_KEEP).all()


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("J", JOINTS)
def test_one_batch_of_mixed_person_counts(J, soft):
    """all 44 images of a set (0 ... 200 persons, the 0-person image included) in ONE launch: what the per-image runs / the reference give"""
    f = fixture()
    for thr, vis in combos(f):
        d = image_set(f, J, thr, vis)
        keep = d["keep_soft" if soft else "keep_hard"]
        score, rank, n_keep = _raw_of(d).run(vis, thr, soft).outputs()
        assert np.array_equal(n_keep, [len(k) for k in keep])
        assert np.array_equal(rank, ranks_of(keep, d["length"]))
        assert np.array_equal(_bits(score), _bits(d["score"].astype(np.float32)))
    # the same batch through the Python surface, length as a list and as a device tensor
    t = lambda a: torch.from_numpy(a).cuda()
    for length in (d["length"], torch.tensor(d["length"], dtype=torch.int32, device="cuda")):
        got = caller.rescore_nms(t(d["preds"]), t(d["maxvals"])[:, :, None], t(d["scale"]), t(d["box_score"]), length, vis, thr, soft=soft)
        assert np.array_equal(got.rank.cpu().numpy(), rank) and np.array_equal(got.n_keep.cpu().numpy(), n_keep)
        assert np.array_equal(_bits(got.score.cpu().numpy()), _bits(score))


def test_a_thousand_persons_in_one_image():
    """the size limit: 1024 persons of one image (bit rows fill 128 KB of LDS, key points stay in global memory) against the restatement;
    persons on a coarse grid of well separated clusters, so every OKS is far from the threshold"""
    rng = np.random.default_rng(5)
    P, J, n_cl = 1024, 17, 400
    base = (np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(n_cl, 1, 2) * 2000.0 + rng.uniform(-50, 50, (n_cl, J, 2)))
    cl = rng.integers(0, n_cl, P)
    preds = (base[cl] + rng.choice([0.0, 0.25], (P, 1, 1)) * rng.standard_normal((P, J, 2))).astype(np.float32)
    maxvals = rng.uniform(0.3, 1.0, (P, J)).astype(np.float32)
    box = rng.permutation(P).astype(np.float32) / P * 0.5 + 0.5       # distinct box scores
    area = np.full(P, 40000.0, np.float32)
    sig = np.asarray(caller.SIGMAS[J])
    for soft in (False, True):
        want = _nms_ref.run_batch(preds, maxvals, area, box, [P], sig, 0.2, 0.9, soft=soft)
        score, rank, n_keep = Raw(preds, maxvals, box, [P], sig, area=area).run(0.2, 0.9, soft).outputs()
        assert len(set(want[0].tolist())) == P
        assert np.array_equal(_bits(score), _bits(want[0])) and np.array_equal(rank, want[1]) and np.array_equal(n_keep, want[2])
        assert 0 < n_keep[0] < P


def test_oks_visibility_threshold_is_the_candidates_mask():
    """the optional in_vis_thre of oks_nms: nms.py:95 evaluates to the CANDIDATE's mask alone; no selected joint: OKS 0 (never suppressed)"""
    f = fixture()
    J, thr, vis, oks_vis = 17, 0.5, 0.2, 0.5
    d = image_set(f, J, thr, vis)
    hi = 41                                               # the images of 0 ... 40 persons
    S = int(np.sum(d["length"][:hi]))
    margins, o = [], 0
    for n in d["length"][:hi]:
        kp = np.concatenate([d["preds"][o:o + n], d["maxvals"][o:o + n][:, :, None]], 2)
        _nms_ref.oks_nms(kp, d["score"][o:o + n], d["area"][o:o + n], thr, d["sigmas"], oks_vis, margins=margins)
        o += n
    assert min(margins) > 1e-6, "an input property: the restatement's own comparisons are not on the threshold"
    masked_out = (d["maxvals"][:S] > np.float32(oks_vis)).sum(1) == 0
    assert masked_out.any(), "the inputs hold persons without a joint above the OKS threshold"
    for soft in (False, True):
        want = _nms_ref.run_batch(d["preds"][:S], d["maxvals"][:S], d["area"][:S], d["box_score"][:S], d["length"][:hi], d["sigmas"], vis, thr,
                                  soft=soft, oks_vis_thre=oks_vis)
        plain = _nms_ref.run_batch(d["preds"][:S], d["maxvals"][:S], d["area"][:S], d["box_score"][:S], d["length"][:hi], d["sigmas"], vis, thr, soft=soft)
        assert not np.array_equal(want[1], plain[1]), "the mask changes the outcome on these inputs"
        score, rank, n_keep = _raw_of(d).run(vis, thr, soft, 0, hi, oks_vis_thre=oks_vis).outputs()
        assert np.array_equal(rank[:S], want[1]) and np.array_equal(n_keep[:hi], want[2]) and np.array_equal(_bits(score[:S]), _bits(want[0]))
        if not soft:
            assert (rank[:S][masked_out] >= 0).all()


def test_equal_scores_lower_crop_index_first():
    J, P = 14, 70                                         # more than one 64-bit word of persons
    rng = np.random.default_rng(1)
    preds = (rng.uniform(0, 50, (1, J, 2)) + np.arange(P).reshape(P, 1, 1) * 1000.0).astype(np.float32)  # far apart: all kept
    preds[5] = preds[4]                                   # ... but 5 duplicates 4 and 69 duplicates 2
    preds[69] = preds[2]
    maxvals = np.full((P, J), 0.5, np.float32)
    box = np.full(P, 0.75, np.float32)
    area = np.full(P, 40000.0, np.float32)
    sig = np.asarray(caller.SIGMAS[J])
    raw = Raw(preds, maxvals, box, [P], sig, area=area)
    s1, r1, k1 = [a.copy() for a in raw.run(0.2, 0.9, False).outputs()]
    raw.reset()
    s2, r2, k2 = raw.run(0.2, 0.9, False).outputs()
    assert np.array_equal(r1, r2) and np.array_equal(k1, k2) and np.array_equal(_bits(s1), _bits(s2))
    assert (s1 == np.float32(0.375)).all() and k1[0] == P - 2
    kept = [p for p in range(P) if p not in (5, 69)]
    assert r1[5] == -1 and r1[69] == -1 and np.array_equal(r1[kept], np.arange(P - 2))
    want = _nms_ref.run_batch(preds, maxvals, area, box, [P], sig, 0.2, 0.9)
    assert np.array_equal(r1, want[1])
    raw.reset()
    s3, r3, k3 = raw.run(0.2, 0.9, True).outputs()       # soft: the first 20 in index order (duplicates decay to below the rest)
    want = _nms_ref.run_batch(preds, maxvals, area, box, [P], sig, 0.2, 0.9, soft=True)
    assert np.array_equal(r3, want[1]) and k3[0] == 20 and np.array_equal(np.sort(r3[r3 >= 0]), np.arange(20))


def test_size_errors_are_codes_not_faults():
    rng = np.random.default_rng(2)
    J, P = 17, 6
    raw = Raw(rng.uniform(0, 500, (P, J, 2)), rng.uniform(0.3, 1, (P, J)), rng.uniform(0.3, 1, P), [P], np.asarray(caller.SIGMAS[J]),
              area=np.full(P, 40000.0))
    raw.run(0.2, 0.9, False, max_persons=1025, expect=-1)
    assert b"over the limit" in cabi.lib().i2r_last_error()
    raw.run(0.2, 0.9, False, n_crops=-3, expect=-1)
    raw.run(0.2, 0.9, False, joints=33, expect=-1)
    score, rank, n_keep = raw.outputs()
    assert (score == np.float32(C_SCORE)).all() and (rank == C_RANK).all() and (n_keep == C_KEEP).all(), "nothing was launched"
    # an image that holds more persons than the host-side bound it was launched with: flagged by the kernel, nothing else written
    score, rank, n_keep = raw.run(0.2, 0.9, False, max_persons=3).outputs()
    assert n_keep[0] == -1 and (score == np.float32(C_SCORE)).all() and (rank == C_RANK).all()
    with pytest.raises(cabi.I2RError, match="over the limit"):
        caller.rescore_nms(torch.zeros(2000, J, 2, device="cuda"), torch.zeros(2000, J, 1, device="cuda"), torch.ones(2000, device="cuda"),
                           torch.ones(2000, device="cuda"), [2000], 0.2, 0.9)
    empty = caller.rescore_nms(torch.zeros(0, J, 2, device="cuda"), torch.zeros(0, J, 1, device="cuda"), torch.ones(0, 2, device="cuda"),
                               torch.ones(0, device="cuda"), [], 0.2, 0.9)
    assert empty.score.numel() == 0 and empty.rank.numel() == 0 and empty.n_keep.numel() == 0
    # no crop at all but two images (a shard whose images hold no person): nothing is launched, every image keeps 0
    torch.full((4096,), 7, dtype=torch.int32, device="cuda")  # (dirty the allocator's free list the outputs come from)
    none = caller.rescore_nms(torch.zeros(0, J, 2, device="cuda"), torch.zeros(0, J, 1, device="cuda"), torch.ones(0, 2, device="cuda"),
                              torch.ones(0, device="cuda"), [0, 0], 0.2, 0.9)
    assert none.score.numel() == 0 and none.n_keep.cpu().tolist() == [0, 0]


def test_scores_equal_as_fp32_are_ordered_by_their_float64_product():
    """the reference sorts the float64 product mean * box_score: persons whose products differ but round to the same fp32 score are
    ordered by value, not by crop index -- here the later crop of every such pair holds the larger product"""
    J = 14
    sig = np.asarray(caller.SIGMAS[J])
    fill = np.float32(0.7)
    mean = np.float32(_nms_ref.rescore(np.full((1, J), fill, np.float32), np.ones(1, np.float32), 0.2)[0])  # fp32 mean of J equal maxima
    pairs, b = [], np.float32(0.75)
    for _ in range(400):    # (a, next float after a) whose products with `mean` round to one fp32 value: about 3 in 10 up here
        nb = np.nextafter(b, np.float32(2))
        if len(pairs) < 8 and np.float32(mean * b) == np.float32(mean * nb):
            pairs.append((b, nb))
            nb = np.nextafter(nb, np.float32(2))
        b = nb
    assert len(pairs) == 8
    box = np.asarray([v for pr in pairs for v in pr], np.float32)   # crop 2k: smaller product, crop 2k + 1: larger
    P = len(box)
    maxvals = np.full((P, J), fill, np.float32)
    preds = (np.arange(P).reshape(P, 1, 1) * 1000.0 + np.zeros((P, J, 2))).astype(np.float32)   # far apart: everyone is kept
    area = np.full(P, 40000.0, np.float32)
    for soft in (False, True):
        want = _nms_ref.run_batch(preds, maxvals, area, box, [P], sig, 0.2, 0.9, soft=soft)
        score, rank, n_keep = Raw(preds, maxvals, box, [P], sig, area=area).run(0.2, 0.9, soft).outputs()
        assert len(set(score.tolist())) == P // 2, "every pair shares its fp32 score"
        assert np.array_equal(_bits(score), _bits(want[0])) and np.array_equal(rank, want[1]) and n_keep[0] == P
        assert all(rank[2 * k + 1] < rank[2 * k] for k in range(P // 2)), "the larger float64 product first, whatever the crop index"


def _duplicated_batch():
    """golden case w48_l31 (3 + 1 crops) with some crops twice: image 0 = crops 0 1 2 + copies of 0 and 1, image 1 = crop 3 + its copy.
    -> cfg, net, x, mask, length, center, scale, box_score, the indices of the copies"""
    cfg, sd, x, m, length, g = setup("w48_l31")
    assert list(length) == [3, 1]
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    src = [0, 1, 2, 0, 1, 3, 3]
    copies = [3, 4, 6]
    center = np.asarray([[300.0 + 700.0 * s, 400.0] for s in src], np.float32)   # persons 700 px apart: OKS of unrelated persons ~ 0
    scale = np.asarray([[1.2, 1.6]] * len(src), np.float32)
    box = np.asarray([0.6 if i in copies else 0.9 for i in range(len(src))], np.float32)
    return cfg, net.cuda(), x[src].cuda(), m[src].cuda(), [5, 2], center, scale, box, copies


def test_end_to_end_forward_flip_decode_nms():
    cfg, net, x, m, length, center, scale, box, copies = _duplicated_batch()
    J = cfg.MODEL.NUM_JOINTS
    y = net.forward_flip(x, m, length, caller.FLIP_PAIRS["crowdpose"])
    preds, maxvals = caller.decode(y, center, scale, cfg.TEST.BLUR_KERNEL)
    for soft in (False, True):
        got = caller.rescore_nms(preds, maxvals, scale, torch.from_numpy(box), length, 0.2, 0.9, soft=soft)
        torch.cuda.synchronize()
        p, mv = preds.cpu().numpy(), maxvals.cpu().numpy()
        area = np.prod(scale * 200, 1)
        want = _nms_ref.run_batch(p, mv, area, box, length, caller.SIGMAS[J], 0.2, 0.9, soft=soft)
        assert (want[0] > 0).all()
        assert np.array_equal(_bits(got.score.cpu().numpy()), _bits(want[0]))
        assert np.array_equal(got.rank.cpu().numpy(), want[1]) and np.array_equal(got.n_keep.cpu().numpy(), want[2])
        if not soft:
            suppressed = np.where(got.rank.cpu().numpy() < 0)[0].tolist()
            assert suppressed == copies, "exactly the lower-scored duplicates are suppressed"
            assert got.n_keep.cpu().tolist() == [3, 1]
    cfg2 = config.load_config("w48_pure_en6", ["TEST.OKS_THRE", "0.9", "TEST.IN_VIS_THRE", "0.2"])
    via_cfg = caller.rescore_nms_cfg(cfg2, preds, maxvals, scale, torch.from_numpy(box), length)
    hard = caller.rescore_nms(preds, maxvals, scale, torch.from_numpy(box), length, 0.2, 0.9)
    assert torch.equal(via_cfg.rank, hard.rank) and torch.equal(via_cfg.score, hard.score) and torch.equal(via_cfg.n_keep, hard.n_keep)
    rows = caller.results(preds, maxvals, hard, length, [11, 12], center, scale)
    assert [len(r) for r in rows] == [3, 1] and [r["image_id"] for r in rows[0]] == [11] * 3
    order = np.argsort(-hard.score.cpu().numpy()[:3]).tolist()
    assert [r["center"] for r in rows[0]] == [center[i].tolist() for i in order]


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


def test_post_step_with_the_nms_hook_equals_the_direct_calls(nccl_world1):
    """dist.PostStep with a decode hook that returns (preds, maxvals, nms): decode + rescoring + OKS-NMS + the all-gather of the packed
    rows on the side stream, three consecutive steps, against the direct calls on the caller's stream"""
    cfg, net, x, m, length, center, scale, box, copies = _duplicated_batch()
    counts = [sum(length)]
    boxt = torch.from_numpy(box).cuda()

    def hook(y):
        preds, maxv = caller.decode(y, center, scale, cfg.TEST.BLUR_KERNEL)
        return preds, maxv, caller.rescore_nms(preds, maxv, scale, boxt, length, 0.2, 0.9)
    step = i2r_dist.PostStep(torch.device("cuda", 0), counts, decode=hook)
    xs = [x * s for s in (1.0, 0.5, 0.25)]
    hs = []
    for xi in xs:
        hs.append(step(net(xi, m, length)))
    last = step.result()
    torch.cuda.synchronize()
    for i, xi in enumerate(xs):
        preds, maxv, nms = hook(net(xi, m, length))
        rows = last if i == len(xs) - 1 else hs[i].out
        kp, score, rank = i2r_dist.unpack_poses(rows.view(counts[0], -1))
        assert torch.equal(kp, torch.cat([preds, maxv], 2)) and torch.equal(score, nms.score) and torch.equal(rank, nms.rank)
        assert torch.equal(i2r_dist.gather_poses(preds, maxv, nms, counts), rows.view(counts[0], -1))
