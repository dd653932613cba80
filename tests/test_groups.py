"""Person groups of the reference's grouped test modes, host side: the numpy restatement tests/_groups_ref.py against the reference
collater's own output (tests/golden/groups_reference.json, tools/make_golden_groups.py), the documented behaviour on shared anchors,
the layout that follows from the person counts alone, and the argument checks of i2r_group_nearest (no device is touched)."""
import json
import os

import numpy as np
import pytest

import _groups_ref
from _golden import GOLDEN
from i2r_amd import cabi
from i2r_amd import input as i2r_input


def fixture():
    with open(os.path.join(GOLDEN, "groups_reference.json")) as f:
        return json.load(f)


def test_fixture_holds_the_stated_inputs():
    fx = fixture()
    a = np.asarray(fx["anchors"], dtype=np.float64)
    assert fx["counts"] == [1, 2, 3, 5, 8, 64, 65, 130] and a.shape == (sum(fx["counts"]), 2)
    assert sorted(c["max_patch"] for c in fx["cases"]) == [1, 2, 3, 7]
    assert (a * 4 == np.round(a * 4)).all() and a.min() >= 0 and a.max() < 4096, "quarter-pixel grid below 4096: every d is exact"
    s = 0
    ties = 0
    for n in fx["counts"]:
        img = a[s:s + n]
        assert len({tuple(r) for r in img}) == n, "no shared anchors"
        for t in range(n):
            d = ((img[t] - img) ** 2).sum(1)
            d = np.delete(d, t)
            ties += len(d) - len(np.unique(d))
        s += n
    assert ties >= 6, "planted equal-distance pairs between non-target persons"


@pytest.mark.parametrize("p", [1, 2, 3, 7])
def test_restatement_equals_the_reference_collater(p):
    fx = fixture()
    case = next(c for c in fx["cases"] if c["max_patch"] == p)
    groups, glen = _groups_ref.main_target(fx["anchors"], fx["counts"], p)
    assert groups == case["main_target"]["groups"]
    assert glen == case["main_target"]["length"]
    assert case["main_target"]["targets"] == [g[0] for g in groups] == list(range(sum(fx["counts"])))
    assert _groups_ref.window(fx["counts"], p) == case["window"]["length"]
    assert case["window"]["index"] == list(range(sum(fx["counts"]))), "window mode keeps the crops in order"
    assert i2r_input.window_lengths(fx["counts"], p) == case["window"]["length"]


def test_shared_anchors_target_first_then_distance_then_index():
    """the one deliberate difference to the reference: with shared anchors its stable sort may put another person in front of the target
    (or cut the target out); here the target is first, always a member, the rest ordered by (d, index)"""
    two = np.array([[10.0, 20.0], [10.0, 20.0]])
    for p in (1, 2, 3):
        groups, glen = _groups_ref.main_target(two, [2], p)
        assert groups == ([[0], [1]] if p == 1 else [[0, 1], [1, 0]])
    five = np.array([[7.25, 9.5]] * 5)
    groups, glen = _groups_ref.main_target(five, [5], 3)
    assert groups == [[0, 1, 2], [1, 0, 2], [2, 0, 1], [3, 0, 1], [4, 0, 1]] and glen == [3] * 5
    # shared pair next to a distinct person: (d, index) behind the target
    mix = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [3.0, 4.0]])
    groups, _ = _groups_ref.main_target(mix, [4], 3)
    assert groups == [[0, 2, 1], [1, 3, 0], [2, 0, 1], [3, 1, 0]]
    for g, t in zip(groups, range(4)):
        assert g[0] == t and len(set(g)) == len(g)


@pytest.mark.parametrize("p", [1, 2, 3, 7, 64])
def test_layout_follows_from_the_person_counts_alone(p):
    length = [1, 2, 3, 5, 64, 65, 130, 1]
    glen, poff, moff = i2r_input.group_layout(length, p)
    assert (glen, poff, moff) == _groups_ref.layout(length, p)
    assert len(glen) == sum(length) and poff[-1] == sum(length) and moff[-1] == sum(glen)
    want = [k for n in length for k in [1 if n == 1 else min(n, p)] * n]
    assert glen == want
    a = _groups_ref.mixed_anchors(length, seed=3)
    groups, glen2 = _groups_ref.main_target(a, length, p)
    assert glen2 == glen
    flat = [i for g in groups for i in g]
    for b in range(len(length)):  # an image's slots hold that image's persons only
        assert all(poff[b] <= i < poff[b + 1] for i in flat[moff[b]:moff[b + 1]])


def test_window_lengths():
    assert i2r_input.window_lengths([1, 2, 7, 8, 15], 7) == [1, 2, 7, 7, 1, 7, 7, 1]
    assert i2r_input.window_lengths([3, 4], 1) == [1] * 7
    assert i2r_input.window_lengths([], 3) == []


@pytest.mark.parametrize("bad", [0, -1])
def test_max_patch_below_one_raises(bad):
    with pytest.raises(ValueError):
        i2r_input.group_layout([2, 3], bad)
    with pytest.raises(ValueError):
        i2r_input.window_lengths([2, 3], bad)
    with pytest.raises(ValueError):
        _groups_ref.main_target(np.zeros((5, 2)), [2, 3], bad)
    with pytest.raises(ValueError):
        i2r_input.main_target_groups(np.zeros((5, 4)), [2, 3], bad, device="cuda:0")  # (refused before a device is touched)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    """null pointers, max_patch < 1, max_patch > 64, negative counts: I2R_E_ARG with a text before anything touches a device (none is
    here); no persons: I2R_OK at once"""
    L = cabi.load_library()
    assert "i2r_group_nearest" in cabi.EXPORTS
    one = 0x1000  # never dereferenced: every case fails its argument check first
    good = dict(anchors=one, person_off=one, member_off=one, n_img=1, n_persons=4, n_members=8, max_patch=2, members=one)

    def call(**kw):
        a = dict(good, **kw)
        return L.i2r_group_nearest(a["anchors"], a["person_off"], a["member_off"], a["n_img"], a["n_persons"], a["n_members"], a["max_patch"],
                                   a["members"], None)
    for bad in (dict(max_patch=0), dict(max_patch=-3), dict(max_patch=65), dict(anchors=None), dict(person_off=None), dict(member_off=None),
                dict(members=None), dict(n_persons=-1), dict(n_img=-1), dict(n_members=3)):
        assert call(**bad) == -1 and L.i2r_last_error(), bad
    assert call(n_persons=0, n_members=0) == 0, "no persons: I2R_OK without a launch"
    assert call(n_persons=0, n_members=0, anchors=None, members=None) == 0
