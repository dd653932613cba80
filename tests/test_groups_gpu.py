"""-m gpu: i2r_group_nearest through the raw C-ABI against the numpy restatement tests/_groups_ref.py (which tests/test_groups.py
holds equal to the reference collater's own output): the member tables are identical integers."""
import numpy as np
import pytest
import torch

import _groups_ref
from i2r_amd import cabi
from i2r_amd import input as i2r_input

pytestmark = pytest.mark.gpu

GUARD, CANARY = 64, -777
MIXED = [1, 130, 2, 3, 5, 64, 65, 1]  # one launch: every lane-striding case (n < 64, = 64, 65, two full strides + 2) and single persons


def raw(anchors, length, p, expect=0):
    """the raw call with canaries on either side of the table -> members (numpy int32)"""
    dev = torch.device("cuda", 0)
    glen, poff, moff = _groups_ref.layout(length, p)
    a = torch.from_numpy(np.ascontiguousarray(anchors, dtype=np.float64).reshape(-1, 2)).to(dev)
    off = torch.tensor(poff + moff, dtype=torch.int32, device=dev)
    out = torch.full((moff[-1] + 2 * GUARD,), CANARY, dtype=torch.int32, device=dev)
    B = len(length)
    rc = cabi.lib().i2r_group_nearest(a.data_ptr(), off.data_ptr(), off.data_ptr() + 4 * (B + 1), B, poff[-1], moff[-1], p,
                                      out.data_ptr() + 4 * GUARD, torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:GUARD] == CANARY).all() and (o[len(o) - GUARD:] == CANARY).all(), "canary overwritten"
    return o[GUARD:len(o) - GUARD]


@pytest.mark.parametrize("p", [1, 2, 3, 7, 64])
def test_mixed_images_with_ties_equal_the_restatement(p):
    anchors = _groups_ref.mixed_anchors(MIXED, seed=11)  # (planted equal-distance pairs, no shared anchors)
    groups, glen = _groups_ref.main_target(anchors, MIXED, p)
    got = raw(anchors, MIXED, p)
    want = np.asarray([i for g in groups for i in g], dtype=np.int32)
    assert got.shape == want.shape and (got == want).all(), np.flatnonzero(got != want)[:8]
    again = raw(anchors, MIXED, p)
    assert (again == got).all(), "deterministic"


def test_every_distance_tied():
    """persons on a circle of radius 5 around person 0 (3-4-5 lattice points): from person 0 every distance is equal, index decides"""
    ring = [(3, 4), (4, 3), (5, 0), (4, -3), (3, -4), (0, -5), (-3, -4), (-4, -3), (-5, 0), (-4, 3), (-3, 4), (0, 5)]
    anchors = np.array([[100.0, 100.0]] + [[100.0 + x, 100.0 + y] for x, y in ring[::-1]])
    for p in (2, 5, 13):
        groups, _ = _groups_ref.main_target(anchors, [13], p)
        assert groups[0] == list(range(min(p, 13)))
        assert raw(anchors, [13], p).tolist() == [i for g in groups for i in g]


@pytest.mark.parametrize("p", [1, 2, 3, 7])
def test_shared_anchors_keep_the_target_first(p):
    two = np.array([[10.0, 20.0], [10.0, 20.0]])
    five = np.array([[7.25, 9.5]] * 5)
    mix = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [3.0, 4.0]])
    anchors, length = np.concatenate([two, five, mix]), [2, 5, 4]
    groups, glen = _groups_ref.main_target(anchors, length, p)
    got = raw(anchors, length, p).tolist()
    assert got == [i for g in groups for i in g]
    firsts, r = [], 0
    for n in glen:
        firsts.append(got[r])
        assert len(set(got[r:r + n])) == n, "a group never repeats a person"
        r += n
    assert firsts == list(range(11)), "group g belongs to person g, who is its first member"


def test_python_entry_takes_any_float_boxes_and_reads_nothing_back():
    anchors = _groups_ref.mixed_anchors(MIXED, seed=5)
    boxes = np.concatenate([anchors, np.full((len(anchors), 2), 50.0)], axis=1)
    groups, glen = _groups_ref.main_target(anchors, MIXED, 3)
    want = [i for g in groups for i in g]
    for b in (boxes, boxes.tolist(), torch.from_numpy(boxes).cuda(), torch.from_numpy(boxes.astype(np.float32)).cuda(),
              torch.from_numpy(boxes).cuda().half()):  # (quarter pixels below 4096 are exact in fp32; in fp16 only the call form is checked)
        g = i2r_input.main_target_groups(b, MIXED, 3, device="cuda:0")
        assert g.group_len == glen and g.n_groups == sum(MIXED) and g.members.dtype == torch.int32 and g.members.is_cuda
        if not (torch.is_tensor(b) and b.dtype == torch.float16):
            assert g.members.cpu().tolist() == want
    with pytest.raises(ValueError):
        i2r_input.main_target_groups(boxes, MIXED, 65, device="cuda:0")
    with pytest.raises(ValueError):
        i2r_input.main_target_groups(boxes[:5], MIXED, 3, device="cuda:0")


def test_no_persons_launches_nothing():
    assert raw(np.zeros((0, 2)), [], 3).size == 0
    dev = torch.device("cuda", 0)
    out = torch.full((8,), CANARY, dtype=torch.int32, device=dev)
    one = torch.zeros(4, dtype=torch.int32, device=dev)
    rc = cabi.lib().i2r_group_nearest(0, one.data_ptr(), one.data_ptr(), 1, 0, 0, 3, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and (out.cpu().numpy() == CANARY).all()


def test_offsets_that_do_not_describe_the_batch_write_nothing_outside():
    """a member table shorter than the layout asks for (n_members cut): the kernel stays inside [0, n_members)"""
    dev = torch.device("cuda", 0)
    length, p = [5, 3], 3
    anchors = _groups_ref.mixed_anchors(length, seed=2)
    glen, poff, moff = _groups_ref.layout(length, p)
    a = torch.from_numpy(anchors).to(dev)
    off = torch.tensor(poff + moff, dtype=torch.int32, device=dev)
    cut = moff[-1] - 4
    out = torch.full((moff[-1] + GUARD,), CANARY, dtype=torch.int32, device=dev)
    rc = cabi.lib().i2r_group_nearest(a.data_ptr(), off.data_ptr(), off.data_ptr() + 4 * 3, 2, poff[-1], cut, p, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    o = out.cpu().numpy()
    groups, _ = _groups_ref.main_target(anchors, length, p)
    want = [i for g in groups for i in g]
    assert o[:cut].tolist() == want[:cut] and (o[cut:] == CANARY).all()
