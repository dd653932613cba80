"""Generate the fixtures of the grouped test modes by running THE REFERENCE ITSELF on CPU (data only):

  tests/golden/groups_reference.json   the reference collater's own main_target and window output (lib/dataset/collater.py:28-95):
                                       index-carrying stand-in items go through collater(max_patch, mode).get_max_patch, the lists that
                                       come back are the groups.  Person counts 1, 2, 3, 5, 8, 64, 65, 130 in one batch, max_patch 1, 2,
                                       3, 7; anchors on a quarter-pixel grid below 4096 (every squared distance exact in float64), planted
                                       equal-distance pairs between non-target persons, no shared anchors (tests/_groups_ref.mixed_anchors).
  tests/golden/w48_mt_p2_l213.npz      validate_main_target's model output (lib/core/function.py:309-334): the w48_l213 inputs
                                       (config w48_pure_en6, lengths [2, 1, 3], synthetic weights and inputs) grouped by the reference's
                                       collater with max_patch 2 and the boxes below -> 11 crops through the reference model, the
                                       first row of every group kept (get_target_person) -> 6 maps.

Run where the reference exists (oracle/ref_shim.py REF_ROOT):

    python tools/make_golden_groups.py [groups] [model]
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ref_shim  # noqa: E402
from ref_shim import REF_LIB  # noqa: E402
import _groups_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
COUNTS = [1, 2, 3, 5, 8, 64, 65, 130]
PATCHES = [1, 2, 3, 7]
# top-left corners (and sizes, unused by the grouping) of the six persons of w48_mt_p2_l213: image 0 two persons, image 1 one, image 2
# three -- person 1 of image 2 is nearest to both others, persons 0 and 2 are each other's farthest
MT_BOXES = [[40.0, 60.0, 80.0, 200.0], [300.0, 80.0, 90.0, 210.0],
            [10.0, 10.0, 50.0, 120.0],
            [100.0, 50.0, 60.0, 150.0], [160.0, 70.0, 70.0, 160.0], [400.0, 300.0, 50.0, 100.0]]
MT_PATCH = 2


def reference_collater():
    """lib/dataset/collater.py alone (the dataset package's __init__ pulls in cv2 and the dataset classes)"""
    spec = importlib.util.spec_from_file_location("i2r_ref_collater", os.path.join(REF_LIB, "dataset", "collater.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.collater


def stand_in_batch(length, boxes):
    """per image: four lists carrying the persons' GLOBAL indices and a meta with the keys get_max_patch touches"""
    items, s = [], 0
    for n in length:
        idx = list(range(s, s + n))
        meta = dict(image="img", filename="", rotation=0, box=[list(b) for b in boxes[s:s + n]])
        for k in ("joints", "joints_vis", "center", "scale", "imgnum", "score"):
            meta[k] = list(idx)
        items.append((list(idx), list(idx), list(idx), list(idx), meta))
        s += n
    return items


def run_collater(collater, length, boxes, max_patch, mode):
    inp, pm, tg, tw, metas = zip(*stand_in_batch(length, boxes))
    inp, pm, tg, tw, metas = collater(max_patch, mode).get_max_patch(list(inp), list(pm), list(tg), list(tw), list(metas))
    assert [list(g) for g in inp] == [list(g) for g in pm] == [list(g) for g in tg] == [list(g) for g in tw]
    return [[int(i) for i in g] for g in inp], metas


def make_groups():
    collater = reference_collater()
    anchors = _groups_ref.mixed_anchors(COUNTS, seed=7)
    boxes = [[x, y, 50.0, 100.0] for x, y in anchors.tolist()]
    cases = []
    for p in PATCHES:
        groups, metas = run_collater(collater, COUNTS, boxes, p, "main_target")
        # (the metas carry the TARGET of every group: tailor_metas(meta, [target_index]))
        targets = [int(m["joints"][0]) for m in metas]
        assert all(len(m["joints"]) == 1 for m in metas) and targets == list(range(sum(COUNTS)))
        win, _ = run_collater(collater, COUNTS, boxes, p, "window")
        cases.append(dict(max_patch=p, main_target=dict(groups=groups, length=[len(g) for g in groups], targets=targets),
                          window=dict(index=[i for g in win for i in g], length=[len(g) for g in win])))
        print("max_patch %d: %d main_target groups (%d crops), %d windows" % (p, len(groups), sum(len(g) for g in groups), len(win)))
    with open(os.path.join(OUT, "groups_reference.json"), "w") as f:
        json.dump(dict(counts=COUNTS, anchors=anchors.tolist(), cases=cases), f, separators=(",", ":"))


def make_model():
    import i2r_amd  # noqa: F401
    from i2r_amd import config, synth
    collater = reference_collater()
    torch.set_num_threads(8)
    cfg = config.load_config("w48_pure_en6")
    net = ref_shim.build_reference_model(cfg)
    sd = synth.make_state_dict(synth.spec_of(net))
    net.load_state_dict(sd, strict=True)
    x, m, length = synth.make_inputs([2, 1, 3], 256, 192)
    groups, _ = run_collater(collater, length, MT_BOXES, MT_PATCH, "main_target")
    members = [i for g in groups for i in g]
    glen = [len(g) for g in groups]
    assert len(members) == 11 and len(glen) == 6
    idx = torch.tensor(members)
    with torch.no_grad():
        y = net(x[idx], m[idx], glen)
    y = y["multi"] if isinstance(y, dict) else y
    first = torch.cat([r[:1] for r in torch.split(y, glen, dim=0)], dim=0)  # get_target_person (function.py:309-314)
    data = dict(out_multi=first.numpy(), members=np.asarray(members, dtype=np.int64), group_len=np.asarray(glen, dtype=np.int64),
                boxes=np.asarray(MT_BOXES, dtype=np.float64), max_patch=np.asarray([MT_PATCH], dtype=np.int64),
                length=np.asarray(length, dtype=np.int64), hw=np.asarray([256, 192], dtype=np.int64),
                x_checksum=np.asarray([x.double().sum().item(), x.double().abs().sum().item()]),
                mask_checksum=np.asarray([m.double().sum().item()]),
                w_checksum=np.asarray([sum(v.double().abs().sum().item() for v in sd.values() if v.dtype == torch.float32)]))
    np.savez_compressed(os.path.join(OUT, "w48_mt_p2_l213.npz"), **data)
    print("w48_mt_p2_l213: groups %s -> %s, |y| mean %.3f" % (groups, tuple(first.shape), first.abs().mean().item()))


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"groups", "model"}
    os.makedirs(OUT, exist_ok=True)
    if "groups" in which:
        make_groups()
    if "model" in which:
        make_model()
