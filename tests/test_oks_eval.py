"""Keypoint OKS evaluation, the CPU side: the float64 restatement tests/_cocoeval_ref.py (the yardstick: pycocotools is absent, parity with
it is unpinned) is held by hand-derived cases whose numbers stand here as fractions; person_count_groups against levels recorded from
the reference's own ClusterMode (tests/golden/cluster_levels.json, tools/make_golden_oks_groups.py); the C-ABI surface of i2r_oks_match
and i2r_oks_accumulate.  The cases themselves are in tests/_oks_cases.py."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _cocoeval_ref as ref
from _oks_cases import HAND, coco_dict, gt_of
from i2r_amd import cabi, caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(HAND))
def test_restatement_gives_the_hand_derived_numbers(name):
    gts, dts, ids, want = HAND[name]
    got = ref.run(gts, dts, ids).stats
    print(name, got.tolist())
    assert np.abs(got - np.asarray([float(w) for w in want])).max() <= 1e-12, (name, got.tolist(), [float(w) for w in want])


def test_tp_fp_tp_precision_array():
    """the precision array behind AP = (51 + 50 * 2/3) / 101, at every threshold"""
    gts, dts, ids, _ = HAND["tp_fp_tp"]
    e = ref.run(gts, dts, ids)
    p = e.eval["precision"][:, :, 0, 0, 0]
    first = 1.0 / (1.0 + np.spacing(1))   # (tp / (fp + tp + spacing(1)): one ulp below 1; 3 + spacing(1) rounds to 3)
    assert (p[:, :51] == first).all() and (p[:, 51:] == 2.0 / 3.0).all() and (e.eval["recall"][:, 0, 0, 0] == 1.0).all()
    assert (e.eval["precision"][:, :, 0, 2, 0] == -1).all(), "no gt in 'large'"


def test_unknown_image_id_is_refused():
    gts, dts, ids, _ = HAND["exact"]
    with pytest.raises(AssertionError, match="do not correspond"):
        ref.run(gts, [dict(dts[0], image_id=8)], ids)
    gt = caller.GtTable.from_coco(coco_dict(gts, ids), device="cpu")
    with pytest.raises(ValueError, match="do not correspond"):
        caller.oks_eval(gt, [8], torch.zeros(1, 17, 2), torch.ones(1))
    with pytest.raises(cabi.I2RError, match="sigma"):
        caller.oks_eval(caller.GtTable.from_arrays([1], [], np.zeros((0, 5, 3)), [], np.zeros((0, 4)), device="cpu"), [1], torch.zeros(1, 5, 2),
                        torch.ones(1))


# ---- lists of dicts <-> the tables of the C-ABI --------------------------------------------------------------------------------------
def test_gt_table_from_coco():
    """images sorted by id, annotations in file order, flags: bit 0 crowd, bit 1 ignore; the non-person category is dropped"""
    gts = [gt_of(9, 0, 0), gt_of(3, 50, 0, iscrowd=1), gt_of(9, 100, 0, v=0), gt_of(3, 150, 0, area=77.0)]
    d = coco_dict(gts, [9, 3, 5])
    d["annotations"].append(dict(gt_of(5, 0, 0), id=99, category_id=2))
    d["categories"].append(dict(id=2, name="dog"))
    t = caller.GtTable.from_coco(d, device="cpu")
    assert t.image_ids.tolist() == [3, 5, 9] and t.counts.tolist() == [2, 0, 2] and t.off.tolist() == [0, 2, 2, 4]
    assert (t.n_img, t.n_gt, t.joints, t.max_gt) == (3, 4, 17, 2)
    assert t.flags.tolist() == [3, 0, 0, 2] and t.area.tolist() == [2500.0, 77.0, 2500.0, 2500.0]
    assert t.kpts.dtype == torch.float64 and t.kpts[:, 0, 0].tolist() == [50.0, 150.0, 0.0, 100.0]
    assert t.bbox[1].tolist() == [150.0, 0.0, 40.0, 30.0]
    with pytest.raises(ValueError):
        caller.GtTable.from_arrays([1, 1], [], np.zeros((0, 17, 3)), [], np.zeros((0, 4)), device="cpu")
    with pytest.raises(ValueError):
        caller.GtTable.from_arrays([1], [2], np.zeros((1, 17, 3)), [1.0], np.zeros((1, 4)), device="cpu")


def test_default_parameters_are_cocoevals():
    p = ref.Params()
    assert np.array_equal(np.asarray(caller.OKS_THRS), p.iouThrs) and np.array_equal(np.asarray(caller.OKS_REC_THRS), p.recThrs)
    assert np.array_equal(np.asarray(caller.OKS_AREA_RNG), np.asarray(p.areaRng, np.float64))
    assert np.array_equal(np.asarray(caller.SIGMAS[17]), p.kpt_oks_sigmas) and list(caller.OKS_STATS_NAMES) == ref.STATS_NAMES
    assert p.maxDets == [20] and 0.5 in caller.OKS_THRS and 0.75 in caller.OKS_THRS


# ---- cluster levels ------------------------------------------------------------------------------------------------------------------
def test_person_count_groups_equal_the_reference_levels():
    f = json.load(open(os.path.join(ROOT, "tests", "golden", "cluster_levels.json")))
    assert f["counts"] == list(range(41)) and [c["start_points"] for c in f["cases"]] == [[1, 2, 6, 10], [1, 3, 5]]
    for case in f["cases"]:
        grp, names = caller.person_count_groups(f["counts"], case["start_points"])
        assert grp.dtype == torch.int32 and names == ["c%d" % (i + 1) for i in range(len(case["start_points"]))]
        got = [names[g] if g >= 0 else None for g in grp.tolist()]
        assert got == case["levels"]
    assert caller.person_count_groups(torch.tensor([0, 1, 7, 12]))[0].tolist() == [-1, 0, 2, 3]   # the default start points


# ---- surface -------------------------------------------------------------------------------------------------------------------------
NEW = {"i2r_oks_match": ("i2r_oks_match_args", "OksMatchArgs", "oks_len", "reserved"),
       "i2r_oks_accumulate": ("i2r_oks_accumulate_args", "OksAccumulateArgs", "precision", "n_rec")}


def test_entry_points_are_declared_exported_and_abi_stays_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert "i2r_oks_eval.hip" in __graft_entry__.SOURCES
    for name, (_, cls, _, _) in NEW.items():
        assert re.search(r"^I2R_API\s+int\s+%s\s*\(" % name, header, flags=re.M)
        assert name in cabi.EXPORTS and name in __graft_entry__.exported_symbols(cabi.LIB_PATH)
        assert getattr(L, name).argtypes[0]._type_ is getattr(cabi, cls)
    assert sorted(cabi.EXPORTS) == __graft_entry__._declared_exports()


def test_args_layouts_match_the_header(tmp_path):
    """sizeof and the offsets of two late fields of the ctypes mirrors equal the C structs' (a tiny gcc program)"""
    items = [(s, f) for s, _, f1, f2 in NEW.values() for f in (f1, f2)]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "i2r_hip.h"\nint main(void) { printf("%zu %zu ' + "%zu " * len(items)
                   + '\\n", sizeof(i2r_oks_match_args), sizeof(i2r_oks_accumulate_args), '
                   + ", ".join("offsetof(%s, %s)" % it for it in items) + "); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(cabi.OksMatchArgs), ctypes.sizeof(cabi.OksAccumulateArgs)]
    want += [getattr(getattr(cabi, cls), f).offset for _, cls, f1, f2 in NEW.values() for f in (f1, f2)]
    assert got == want


def test_refused_bounds_return_a_code_without_a_launch():
    """max_dets > 32, more than 256 gts / 1024 detections of one image, J > 32, 17 thresholds, 5 area ranges, 129 recall thresholds:
    I2R_E_ARG with a text, before anything touches a device (none is here)"""
    L = cabi.load_library()
    one = 0x1000   # never dereferenced: every case fails its argument check first
    ptrs = dict(dt_kpts=one, dt_score=one, dt_off=one, gt_kpts=one, gt_area=one, gt_bbox=one, gt_flags=one, gt_off=one, sigmas=one, thr=one,
                area_rng=one, dt_rank=one, dt_match=one, dt_ignore=one, gt_ignore=one)
    base = dict(n_dt=4, n_gt=4, n_img=1, joints=17, n_thr=10, n_area=3, max_dets=20, max_dt_per_img=4, max_gt_per_img=4)
    for bad in (dict(max_dets=33), dict(max_dets=0), dict(max_gt_per_img=257), dict(max_dt_per_img=1025), dict(joints=33), dict(joints=0),
                dict(n_thr=17), dict(n_area=5), dict(n_dt=-1), dict(sigmas=None), dict(dt_rank=None), dict(oks=one)):
        a = cabi.OksMatchArgs(**dict(ptrs, **dict(base, **bad)))
        assert L.i2r_oks_match(ctypes.byref(a), None) == -1 and L.i2r_last_error(), bad
    assert L.i2r_oks_match(ctypes.byref(cabi.OksMatchArgs(**dict(base, n_img=0))), None) == 0, "no image: I2R_OK without a launch"
    ptrs = dict(dt_match=one, dt_ignore=one, order=one, dt_img=one, img_group=one, gt_ignore=one, gt_off=one, rec_thr=one, precision=one,
                recall=one, npig=one)
    base = dict(n_dt=4, n_gt=4, n_img=1, n_part=4, n_group=1, n_thr=10, n_area=3, n_rec=101)
    for bad in (dict(n_rec=129), dict(n_rec=0), dict(n_thr=17), dict(n_area=0), dict(n_part=-1), dict(precision=None), dict(order=None),
                dict(img_group=None)):
        a = cabi.OksAccumulateArgs(**dict(ptrs, **dict(base, **bad)))
        assert L.i2r_oks_accumulate(ctypes.byref(a), None) == -1 and L.i2r_last_error(), bad
