"""CPU: rescoring + OKS-NMS -- the float64 restatement against the reference's own output (tests/golden/nms_reference.npz, written by
tools/make_golden_nms.py from the reference's evaluate() / oks_nms / soft_oks_nms), the fixture's recorded conditions, the C-ABI surface
of i2r_pose_nms, and the host-side ends (caller.results, dist.gather_poses)."""
import ctypes
import os
import re
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _nms_ref
from i2r_amd import cabi, caller
from i2r_amd import dist as i2r_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "nms_reference.npz")
JOINTS = (17, 14)


def fixture():
    return np.load(FIX)


def combos(f):
    return [(float(t), float(v)) for t, v in f["combos"]]


def image_set(f, J, thr, vis):
    """-> dict of one (J, oks_thre, in_vis_thre) set: the shared inputs of J + this set's reference outputs, keep lists per image"""
    pre, q = "j%d_" % J, "j%d_t%g_v%g_" % (J, thr, vis)
    d = {k: f[pre + k] for k in ("preds", "maxvals", "center", "scale", "area", "box_score", "sigmas")}
    d["length"] = [int(c) for c in f["counts"]]
    d["score"] = f[q + "score"]
    for name in ("keep_hard", "keep_soft"):
        flat, n = f[q + name].astype(int), f[q + name + "_n"].astype(int)
        cuts = np.concatenate([[0], np.cumsum(n)])
        d[name] = [flat[cuts[i]:cuts[i + 1]].tolist() for i in range(len(n))]
    for name in ("min_oks_margin", "min_soft_gap", "min_score_gap", "max_invisible_persons"):
        d[name] = f[q + name].item()
    return d


def ranks_of(keep_lists, length):
    """the kernel's rank output for the reference's keep lists"""
    rank, o = np.full(sum(length), -1, np.int32), 0
    for keep, n in zip(keep_lists, length):
        for k, p in enumerate(keep):
            rank[o + p] = k
        o += n
    return rank


@pytest.mark.parametrize("J", JOINTS)
def test_restatement_reproduces_the_reference(J):
    """every keep list, hard and soft, and every score cast to float32, of every set"""
    f = fixture()
    assert bool(f["rescoring_from_evaluate"]), "the fixture's scores come from the dataset class's own evaluate()"
    for thr, vis in combos(f):
        d = image_set(f, J, thr, vis)
        o = 0
        for i, n in enumerate(d["length"]):
            sl = slice(o, o + n)
            kp = np.concatenate([d["preds"][sl], d["maxvals"][sl][:, :, None]], 2)
            sc = _nms_ref.rescore(d["maxvals"][sl], d["box_score"][sl], vis)
            assert np.array_equal(sc.astype(np.float32), d["score"][sl].astype(np.float32)), (J, thr, vis, i)
            assert _nms_ref.oks_nms(kp, sc, d["area"][sl], thr, d["sigmas"]) == d["keep_hard"][i], (J, thr, vis, i)
            assert _nms_ref.soft_oks_nms(kp, sc, d["area"][sl], thr, d["sigmas"], max_dets=int(f["max_dets"])) == d["keep_soft"][i], (J, thr, vis, i)
            o += n
        assert np.array_equal(np.prod(d["scale"] * 200, 1), d["area"])  # function.py:220 on float32


@pytest.mark.parametrize("J", JOINTS)
def test_fixture_meets_its_recorded_conditions(J):
    f = fixture()
    assert [int(c) for c in f["counts"]] == list(range(41)) + [64, 100, 200]
    assert sorted(combos(f)) == sorted([(0.9, 0.2), (0.9, 0.0), (0.5, 0.2), (0.5, 0.0)])
    for thr, vis in combos(f):
        d = image_set(f, J, thr, vis)
        assert d["min_oks_margin"] >= 1e-4 and d["min_soft_gap"] >= 1e-4 and d["min_score_gap"] > 0 and d["max_invisible_persons"] <= 1
        margins, gaps, o = [], [], 0
        for i, n in enumerate(d["length"]):  # (a)-(d) re-measured with the restatement
            sl = slice(o, o + n)
            kp = np.concatenate([d["preds"][sl], d["maxvals"][sl][:, :, None]], 2)
            s32 = d["score"][sl].astype(np.float32)
            assert len(set(s32.tolist())) == n                                             # (b)
            assert int(((d["maxvals"][sl] > np.float32(vis)).sum(1) == 0).sum()) <= 1       # (d)
            _nms_ref.oks_nms(kp, d["score"][sl], d["area"][sl], thr, d["sigmas"], margins=margins)
            _nms_ref.soft_oks_nms(kp, d["score"][sl], d["area"][sl], thr, d["sigmas"], gaps=gaps)
            o += n
        assert min(margins) >= 1e-4 and abs(min(margins) - d["min_oks_margin"]) < 1e-9     # (a)
        assert min(gaps) >= 1e-4 and abs(min(gaps) - d["min_soft_gap"]) < 1e-6 * max(1.0, min(gaps))  # (c)
        n_kept = sum(len(k) for k in d["keep_hard"])                                       # (e)
        assert 0 < n_kept < sum(d["length"]), "set (J=%d, thr=%g, vis=%g) holds kept AND suppressed persons" % (J, thr, vis)
        assert any(len(k) == 20 and n > 20 for k, n in zip(d["keep_soft"], d["length"])), "soft form's truncation is exercised"


def test_pose_nms_is_declared_exported_and_abi_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert re.search(r"^I2R_API\s+int\s+i2r_pose_nms\s*\(", header, flags=re.M)
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    assert "i2r_pose_nms" in cabi.EXPORTS
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    assert "i2r_pose_nms" in __graft_entry__.exported_symbols(cabi.LIB_PATH)
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17 and L.i2r_pose_nms.argtypes[0]._type_ is cabi.PoseNmsArgs
    assert "i2r_nms.hip" in __graft_entry__.SOURCES


def test_pose_nms_args_layout_matches_header(tmp_path):
    """sizeof and the offset of the last field of the ctypes mirror equal the C struct's (a tiny gcc program)"""
    import subprocess
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "i2r_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(i2r_pose_nms_args), offsetof(i2r_pose_nms_args, in_vis_thre), offsetof(i2r_pose_nms_args, reserved)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(cabi.PoseNmsArgs), cabi.PoseNmsArgs.in_vis_thre.offset, cabi.PoseNmsArgs.reserved.offset]


def test_sigmas_equal_the_reference_tables():
    f = fixture()
    assert sorted(caller.SIGMAS) == [14, 17]
    for J in JOINTS:
        assert np.array_equal(np.asarray(caller.SIGMAS[J], np.float64), f["j%d_sigmas" % J])


def test_argument_errors_return_a_code_without_a_launch():
    """J > 32, a person count over the limit, null outputs: I2R_E_ARG with a text, before anything touches a device (none is here)"""
    L = cabi.load_library()
    one = 0x1000  # never dereferenced: every case fails its argument check first

    def args(**kw):
        base = dict(preds=one, maxvals=one, scale=one, area=None, box_score=one, img_off=one, sigmas=one, score=one, rank=one, n_keep=one,
                    in_vis_thre=0.2, oks_thre=0.9, oks_vis_thre=0.0, n_crops=4, n_img=1, joints=17, max_persons=4, soft=0, max_dets=20,
                    use_oks_vis=0)
        base.update(kw)
        return cabi.PoseNmsArgs(**base)
    for kw, text in ((dict(joints=33), b"joints"), (dict(joints=0), b"joints"), (dict(max_persons=1025), b"over the limit"),
                     (dict(n_crops=5000, max_persons=5000), b"over the limit"), (dict(score=None), b"null output"),
                     (dict(rank=None), b"null output"), (dict(n_keep=None), b"null output"), (dict(preds=None), b"null input"),
                     (dict(scale=None, area=None), b"null input"), (dict(soft=2), b"soft"), (dict(n_crops=-1), b"n_crops"),
                     (dict(oks_thre=0.0), b"oks_thre")):
        a = args(**kw)
        assert L.i2r_pose_nms(ctypes.byref(a), None) == -1, kw
        assert text in L.i2r_last_error(), (kw, L.i2r_last_error())
    assert L.i2r_pose_nms(None, None) == -1
    # nothing to do: returns at once, with no device and null pointers
    for kw in (dict(n_crops=0, max_persons=0), dict(n_img=0)):
        a = args(preds=None, score=None, **kw)
        assert L.i2r_pose_nms(ctypes.byref(a), None) == 0, kw


def _nms_of(rank, score):
    return types.SimpleNamespace(rank=rank, score=score)


def _poses_worker(rank, world, port, counts):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        S, J = sum(counts), 5
        g = torch.Generator().manual_seed(3)
        preds = torch.randn(S, J, 2, generator=g)
        maxv = torch.rand(S, J, 1, generator=g)
        score = torch.rand(S, generator=g)
        rk = (torch.arange(S, dtype=torch.int32) % 4) - 1   # -1, 0, 1, 2, ...
        off = sum(counts[:rank])
        sl = slice(off, off + counts[rank])
        for async_op in (False, True):
            rows = i2r_dist.gather_poses(preds[sl], maxv[sl], _nms_of(rk[sl], score[sl]), counts, async_op=async_op)
            if async_op:
                rows = rows.wait()
            assert rows.shape == (S, J * 3 + 2)
            kp, sc, r = i2r_dist.unpack_poses(rows)
            assert torch.equal(kp, torch.cat([preds, maxv], 2)) and torch.equal(sc, score)
            assert r.dtype == torch.int32 and torch.equal(r, rk)
    finally:
        dist.destroy_process_group()


def test_gather_poses_world2_gloo():
    for counts in ([5, 2], [3, 0], [0, 4]):   # uneven shards, one empty shard
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        mp.spawn(_poses_worker, args=(2, port, counts), nprocs=2, join=True)


@pytest.mark.parametrize("soft", [False, True])
def test_results_rows_in_the_reference_order(soft):
    """caller.results on host tensors: per image the fixture's keep order, rows shaped like _coco_keypoint_results_one_category_kernel's"""
    f = fixture()
    J, thr, vis = 17, 0.9, 0.2
    d = image_set(f, J, thr, vis)
    keep = d["keep_soft" if soft else "keep_hard"]
    length = d["length"]
    nms = _nms_of(torch.from_numpy(ranks_of(keep, length)), torch.from_numpy(d["score"].astype(np.float32)))
    ids = [1000 + i for i in range(len(length))]
    rows = caller.results(torch.from_numpy(d["preds"]), torch.from_numpy(d["maxvals"])[:, :, None], nms, length, ids, d["center"], d["scale"])
    assert len(rows) == len(length)
    o = 0
    for i, n in enumerate(length):
        assert len(rows[i]) == len(keep[i])
        for row, p in zip(rows[i], keep[i]):
            assert sorted(row) == ["center", "image_id", "keypoints", "scale", "score"] and row["image_id"] == ids[i]
            want = np.concatenate([d["preds"][o + p], d["maxvals"][o + p][:, None]], 1).reshape(-1)
            assert np.array_equal(np.asarray(row["keypoints"], np.float32), want) and len(row["keypoints"]) == J * 3
            assert np.float32(row["score"]) == np.float32(d["score"][o + p])
            assert row["center"] == d["center"][o + p].tolist() and row["scale"] == d["scale"][o + p].tolist()
        o += n


def test_config_variant_reads_the_thresholds():
    """rescore_nms_cfg hands TEST.IN_VIS_THRE / OKS_THRE / SOFT_NMS and MODEL.NUM_JOINTS on (the reference's yamls: 0.9 and 0.2)"""
    from i2r_amd import config
    cfg = config.load_config("w48_pure_en6", ["TEST.OKS_THRE", "0.9", "TEST.IN_VIS_THRE", "0.2"])
    assert (cfg.TEST.OKS_THRE, cfg.TEST.IN_VIS_THRE, cfg.TEST.SOFT_NMS, cfg.MODEL.NUM_JOINTS) == (0.9, 0.2, False, 14)
    seen = {}

    def fake(preds, maxvals, sa, box, length, in_vis_thre, oks_thre, soft=False, **kw):
        seen.update(in_vis_thre=in_vis_thre, oks_thre=oks_thre, soft=soft)
        return "r"
    real, caller.rescore_nms = caller.rescore_nms, fake
    try:
        assert caller.rescore_nms_cfg(cfg, torch.zeros(2, 14, 2), None, None, None, [2]) == "r"
        with pytest.raises(AssertionError):
            caller.rescore_nms_cfg(cfg, torch.zeros(2, 17, 2), None, None, None, [2])
    finally:
        caller.rescore_nms = real
    assert seen == dict(in_vis_thre=0.2, oks_thre=0.9, soft=False)
