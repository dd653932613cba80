"""CPU: the layout arithmetic of an attention-map capture (i2r_amd.attn_capture: plan() of the three forms) against a restatement of the
formulas in the comments of i2r_attn_weights_args / i2r_attn_query_args / i2r_attn_person_args (include/i2r_hip.h), written here as plain
loops that share no code with the package, and against literals worked by hand.  No GPU, no built library: a wrong stride or tile count
would be an out-of-bounds workspace access on the device, so it is caught here."""
import os
import subprocess
import sys

import pytest
import torch

from i2r_amd.attn_capture import AttnQueries, FullForm, PersonForm, PersonMaps, QueryForm, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST = "enc"
CAP = frozenset({(ST, 0), (ST, 1)})  # two captured layers


# ---- the header, restated ----
def _ceil(a, b):
    q = 0
    while q * b < a:
        q += 1
    return q


def header(kind, lens, heads, mode=0, scale=1, hw=1, K=0, cnt=None):
    """-> dict(stride, ws_rows: workspace rows of ws_stride floats, rows, n_tiles, n_col_tiles, sizes: per block set the floats of every group's block)"""
    longest = total = 0
    for n in lens:
        longest, total = max(longest, n), total + n
    stride = 2 * heads * _ceil(longest, 128)           # ws_stride >= 2 * heads * ceil(max L_g / 128)
    full_tiles = 0
    for n in lens:                                      # one wave per (16-query tile, 128-key block)
        full_tiles += _ceil(n, 16) * _ceil(n, 128)
    if kind == "full":                                  # ws: ws_stride floats per token row; blocks [L_g, L_g]
        return dict(stride=stride, ws_rows=total, rows=0, n_tiles=full_tiles, n_col_tiles=0, sizes=[[n * n for n in lens]])
    if kind == "query":
        tiles = cols = 0
        for n, c in zip(lens, cnt):
            tiles += _ceil(c, 16) * _ceil(n, 128)       # mode 0: sum of ceil(K_g / 16) * ceil(L_g / 128)
            cols += _ceil(n, 16) * _ceil(c, 16)         # mode 1: sum of ceil(L_g / 16) * ceil(K_g / 16)
        return dict(stride=stride, ws_rows=len(lens) * K if mode == 0 else total,  # mode 0: n_grp * K rows; mode 1: per token row
                    rows=K * total if scale > 1 else 0,  # scale > 1 only: K * grp_off[n_grp] floats
                    n_tiles=tiles if mode == 0 else full_tiles, n_col_tiles=cols if mode == 1 else 0,
                    sizes=[[c * n * scale * scale for n, c in zip(lens, cnt)]])  # [K_g, P_g, h scale, w scale] = K_g L_g scale^2
    pmax = 0
    for n in lens:
        assert n % hw == 0
        pmax = max(pmax, n // hw)
    rows = pmax * total * (2 if mode == 1 and scale > 1 else 1)  # Pmax * grp_off[n_grp]; twice that for mode 1 at scale > 1
    return dict(stride=stride, ws_rows=total, rows=rows, n_tiles=0, n_col_tiles=0,
                sizes=[[(n // hw) ** 2 for n in lens], [(n // hw) * n * scale * scale if mode else 0 for n in lens]])


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def intervals(plan, n_layers):
    """[first, last) floats of every view in a buffer of n_layers layers laid out by plan, and the buffer's floats"""
    out = []
    for j in range(n_layers):
        for blk in plan.blocks:
            for g, s in enumerate(blk.shapes or []):
                first = j * plan.layer_floats + blk.base + blk.offs[g]
                out.append((first, first + _numel(s)))
    return out, n_layers * plan.layer_floats


def check_against_header(plan, want, n_layers=2):
    assert plan.ws_stride >= want["stride"] and plan.ws_floats >= want["ws_rows"] * plan.ws_stride and plan.rows_floats >= want["rows"]
    assert (plan.n_tiles, plan.n_col_tiles) == (want["n_tiles"], want["n_col_tiles"])
    assert plan.layer_floats % 4 == 0, "layers must start on 16-byte boundaries"
    assert len(plan.blocks) == len(want["sizes"])
    for blk, sizes in zip(plan.blocks, want["sizes"]):
        assert blk.base % 4 == 0 and [blk.offs[g + 1] - blk.offs[g] for g in range(len(sizes))] == sizes
        assert blk.shapes is None and not any(sizes) or [_numel(s) for s in blk.shapes] == sizes
    iv, total = intervals(plan, n_layers)
    iv.sort()
    assert iv[0][0] >= 0 and iv[-1][1] <= total, "a view outside the buffer"
    assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:])), "two views overlap"


# ---- the cases ----
def _tokens(lens, K, cnt):
    return torch.tensor([[(7 * k) % n if k < c else -1 for k in range(K)] for n, c in zip(lens, cnt)], dtype=torch.int32)


def _query(mode, scale, lens, K, cnt=None, tok=None):
    q = AttnQueries({ST: _tokens(lens, K, cnt or [K] * len(lens)) if tok is None else tok}, mode, scale, {ST: cnt} if cnt else None)
    return QueryForm(CAP, q), q


def check_literals():
    p = FullForm(CAP).plan(ST, (5, 6), [30, 17], 2)
    assert (p.n_grp, p.ws_stride, p.ws_floats, p.blocks[0].offs[:-1], p.layer_floats, p.n_tiles) == (2, 4, 188, [0, 900], 1192, 4)
    assert p.blocks[0].shapes == [(30, 30), (17, 17)] and intervals(p, 2)[0][2] == (1192, 1192 + 900)  # (layer 1's views start at 1192)
    p = FullForm(CAP).plan(ST, (10, 13), [130], 8)
    assert (p.ws_stride, p.n_tiles, p.layer_floats) == (32, 18, 16900)
    two = [FullForm(CAP).plan(ST, (1, 1), [130], 8), FullForm(CAP).plan(ST, (1, 1), [30, 17], 2)]
    FullForm.share(two)  # (the launches of both stacks read one stride)
    assert [(p.ws_stride, p.ws_floats) for p in two] == [(32, 130 * 32)] * 2

    lens, cnt = [24, 12], [5, 3]
    f, q = _query(0, 2, lens, 5, cnt)
    p = f.plan(ST, (3, 4), lens, 2, q)
    assert (p.ws_stride, p.ws_floats, p.rows_floats, p.blocks[0].offs[:-1], p.layer_floats) == (4, 40, 180, [0, 480], 624)
    assert (p.n_tiles, p.n_col_tiles, p.K, p.blocks[0].shapes) == (2, 0, 5, [(5, 2, 6, 8), (3, 1, 6, 8)])
    assert torch.equal(p.tables[0], q.tokens[ST]) and p.tables[1].tolist() == cnt and p.tables[1].dtype == torch.int32
    f, q = _query(1, 2, lens, 5, cnt)
    p = f.plan(ST, (3, 4), lens, 2, q)
    assert (p.ws_floats, p.n_tiles, p.n_col_tiles) == (144, 3, 3)
    f, q = _query(0, 1, lens, 5, cnt)
    assert f.plan(ST, (3, 4), lens, 2, q).rows_floats == 1

    lens = [36, 12]
    p = PersonForm(CAP, PersonMaps(2, 2)).plan(ST, (3, 4), lens, 2)
    assert (p.ws_stride, p.ws_floats, p.rows_floats, p.layer_floats) == (4, 192, 144, 492)
    rel, maps = p.blocks
    assert (rel.offs[:-1], rel.base, maps.offs[:-1], maps.base, maps.offs[-1]) == ([0, 9], 0, [0, 432], 12, 480)
    assert rel.shapes == [(3, 3), (1, 1)] and maps.shapes == [(3, 3, 6, 8), (1, 1, 6, 8)]
    assert PersonForm(CAP, PersonMaps(1, 2)).plan(ST, (3, 4), lens, 2).rows_floats == 288
    p = PersonForm(CAP, PersonMaps(0, 2)).plan(ST, (3, 4), lens, 2)
    assert p.layer_floats == 12 and p.blocks[1].shapes is None and p.blocks[1].offs == [0, 0, 0]


# (token map 3 x 4; groups in persons) one group, ragged groups, exactly 128 and 129 tokens with hw 1, a single-token group
GROUPINGS = [((3, 4), [2]), ((3, 4), [3, 1, 2, 5]), ((1, 1), [128]), ((1, 1), [129]), ((1, 1), [1]), ((1, 1), [1, 129, 16, 17]), ((2, 8), [8, 1, 9])]


def check_properties():
    for (h, w), pers in GROUPINGS:
        lens = [n * h * w for n in pers]
        for heads in (1, 3):
            check_against_header(FullForm(CAP).plan(ST, (h, w), lens, heads), header("full", lens, heads))
            for scale in (1, 2):
                for K, cnt in ((1, None), (5, None), (19, [1 + (3 * g) % min(19, n) for g, n in enumerate(lens)])):  # (counts below K)
                    for mode in (0, 1):
                        f, q = _query(mode, scale, lens, K, cnt)
                        p = f.plan(ST, (h, w), lens, heads, q)
                        check_against_header(p, header("query", lens, heads, mode, scale, h * w, K, cnt or [K] * len(lens)))
                        assert [s[0] for s in p.blocks[0].shapes] == (cnt or [K] * len(lens))
                for mode in (0, 1, 2):
                    p = PersonForm(CAP, PersonMaps(mode, scale)).plan(ST, (h, w), lens, heads)
                    check_against_header(p, header("person", lens, heads, mode, scale, h * w))


def check_rejections():
    lens = [24, 12]
    for tok in (torch.zeros(5, dtype=torch.int32), torch.zeros(2, 5, 1, dtype=torch.int32), torch.zeros(3, 5, dtype=torch.int32),
                torch.zeros(1, 5, dtype=torch.int32)):  # wrong rank, wrong number of groups
        f, q = _query(0, 1, lens, 5, tok=tok)
        with pytest.raises(ValueError, match="query tokens of 'enc': shape"):
            f.plan(ST, (3, 4), lens, 2, q)
    for cnt in ([0, 3], [5, 6], [5]):  # a count of 0, above K, one count too few
        f, q = _query(0, 1, lens, 5, cnt, tok=torch.zeros(2, 5, dtype=torch.int32))
        with pytest.raises(ValueError, match="query counts of 'enc'"):
            f.plan(ST, (3, 4), lens, 2, q)
    f, q = _query(1, 2, lens, 5, tok=torch.tensor([[0, 1, 2, 3, 23], [0, 1, 12, 3, 4]], dtype=torch.int32))  # 12 = its group's length
    with pytest.raises(ValueError, match="query token 12 of group 1 of 'enc' is outside its 12 tokens"):
        f.plan(ST, (3, 4), lens, 2, q)
    f, q = _query(1, 2, lens, 5, [5, 2], tok=torch.tensor([[0, 1, 2, 3, 23], [0, 11, 12, 3, 4]], dtype=torch.int32))  # (behind the count: unread)
    f.plan(ST, (3, 4), lens, 2, q)
    f, q = _query(0, 2, [24, 13], 5)
    with pytest.raises(AssertionError):  # a length that is no multiple of h w
        f.plan(ST, (3, 4), [24, 13], 2, q)
    with pytest.raises(AssertionError):
        PersonForm(CAP, PersonMaps(0, 1)).plan(ST, (3, 4), [24, 13], 2)


def check_all():
    check_literals()
    check_properties()
    check_rejections()


def test_plan_literals():
    check_literals()


def test_plan_properties_against_the_header():
    check_properties()


def test_plan_rejections():
    check_rejections()


def test_forms_and_their_program_keys():
    stacks = {"single": 4, "inter": 6}
    args = (stacks, "inter", False)
    assert resolve(None, None, None, None, *args) is None and resolve((), None, None, "flip", *args) is None
    cap = {("inter", 0), ("single", 3)}
    f = resolve(cap, None, None, None, *args)
    assert type(f) is FullForm and f.capture == frozenset(cap) and f.key == ("capture", frozenset(cap)) and f.call is None
    q = AttnQueries({"inter": torch.zeros(2, 7), "single": torch.zeros(4, 3)}, "affect", {"inter": 16, "single": 4}, capacity=9)
    f = resolve(cap, q, None, None, *args)
    assert type(f) is QueryForm and f.key == ("capture", frozenset(cap), "query", 1, 9, (("inter", 16), ("single", 4))) and f.call is q
    f = resolve({("inter", 5)}, None, PersonMaps("affect", 16), None, *args)
    assert type(f) is PersonForm and f.key == ("capture", frozenset({("inter", 5)}), "persons", 2, 16) and f.N_BLOCKS == 2
    for bad, match in (((cap, None, PersonMaps(), None), "not this model's inter-human stack"), (({("inter", 0)}, q, PersonMaps(), None), "not with"),
                       (({("inter", 0)}, None, PersonMaps(), "flip"), "not with"), ((None, None, PersonMaps(), None), "needs capture"),
                       ((None, q, None, None), "needs capture"), (({("inter", 6)}, None, None, None), "encoder stacks are"),
                       (({("inter", 0)}, AttnQueries({"single": torch.zeros(4, 3)}), None, None), "no table for"),
                       (({("inter", 0)}, AttnQueries({"inter": torch.zeros(4, 3)}, upsample=65), None, None), "upsample")):
        with pytest.raises(ValueError, match=match):
            resolve(*bad, *args)
    with pytest.raises(ValueError, match="ATTENTION_TYPE window"):
        resolve({("inter", 0)}, None, PersonMaps(), None, stacks, "inter", True)
    with pytest.raises(ValueError, match="not this model's inter-human stack None"):
        resolve({("inter", 0)}, None, PersonMaps(), None, {"single": 4}, "inter", False)
    with pytest.raises(AssertionError):
        resolve(cap, None, None, "flip", *args)


def test_every_form_names_its_work_behind_the_head_and_its_entry_point():
    """every form resolve() can return: `behind` is one of the four values and attn_bind has a bind / run pair for it, `entry` is an
    exported C entry point, and the flags the other tests read keep their values (deferred, merged, per_stack, N_BLOCKS)"""
    from i2r_amd import attn_bind, cabi
    from i2r_amd.attn_capture import JointQueries, Rollout, TargetMaps
    stacks = {"single": 4, "inter": 6}
    cap, inter = {("inter", 0), ("inter", 1), ("single", 3)}, {("inter", 2), ("inter", 3)}
    tok = {"inter": torch.zeros(2, 7, dtype=torch.int32), "single": torch.zeros(4, 3, dtype=torch.int32)}
    q, j = AttnQueries(tok, "affect", 4), JointQueries()
    res = lambda capture, queries=None, persons=None, flip=None, **kw: resolve(capture, queries, persons, flip, stacks, "inter", False, **kw)  # noqa: E731
    cases = [  # (the call, its form's class name, behind, entry, deferred, merged, per_stack, N_BLOCKS)
        (res(cap), "FullForm", None, "i2r_attn_weights", False, False, False, 1),
        (res(cap, q), "QueryForm", None, "i2r_attn_query_maps", False, False, False, 1),
        (res(inter, persons=PersonMaps("affect", 2)), "PersonForm", None, "i2r_attn_person_maps", False, False, False, 2),
        (res(cap, joints=j, n_joints=17), "JointForm", "launches", "i2r_attn_query_maps", True, False, False, 1),
        (res(cap, flip="flip", joints=j, n_joints=17), "JointForm", "launches", "i2r_attn_query_maps", True, False, False, 1),
        (res(inter, targets=TargetMaps("dependency")), "TargetForm", None, "i2r_attn_target_maps", False, False, False, 2),
        (res(cap, rollout=Rollout(tok)), "RolloutForm", "rollout", "i2r_attn_rollout_step", True, False, True, 2),
        (res(inter, rollout=Rollout(None, "affect")), "RolloutForm", "rollout", "i2r_attn_rollout_step", True, False, True, 3),
        (res(cap, q, flip="flip", flip_maps="merged"), "QueryForm", "merge", "i2r_attn_query_maps", True, True, False, 1),
        (res(inter, persons=PersonMaps("affect", 2), flip="flip", flip_maps="merged"), "PersonForm", "merge", "i2r_attn_person_maps", True, True, False, 2),
        (res(cap, flip="flip", joints=j, n_joints=17, flip_maps="merged"), "JointForm", "merge", "i2r_attn_query_maps", True, True, False, 1),
    ]
    assert set(attn_bind.PAIRS) == {"launches", "merge", "rollout"}
    for f, name, behind, entry, deferred, merged, per_stack, n_blocks in cases:
        assert type(f).__name__ == name
        assert f.behind == behind and f.behind in (None, "launches", "merge", "rollout"), name
        if f.behind is not None:
            bind, run = attn_bind.PAIRS[f.behind]
            assert callable(bind) and callable(run)
        assert f.entry == entry and f.entry in cabi.EXPORTS, name
        assert (f.deferred, f.merged, f.per_stack, f.N_BLOCKS) == (deferred, merged, per_stack, n_blocks), name
        assert (f.J == 17) == (name == "JointForm") and bool(f.behind) == f.deferred
        if f.merged:  # (the fields a merged form's second launch is aimed through are fields of its launch args)
            args = {"i2r_attn_query_maps": cabi.AttnQueryArgs, "i2r_attn_person_maps": cabi.AttnPersonArgs}[f.entry]
            assert len(f.HALF) == 5 and {n for n in f.HALF if n} <= {n for n, _ in args._fields_}


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import torch
import i2r_amd
from i2r_amd import cabi
def touched(*a, **k):
    raise RuntimeError("the planner touched the device or the library")
cabi.lib = cabi.load_library = torch.cuda._lazy_init = torch.cuda.init = touched
import test_attn_capture_plan
test_attn_capture_plan.check_all()
assert cabi._LIB is None and not torch.cuda.is_initialized() and "i2r_amd.engine" not in sys.modules
print("planned in isolation")
"""


def test_planning_needs_no_device_and_no_library():
    """the plan cases first thing in a fresh interpreter in which loading the library or initialising the device raises"""
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "planned in isolation" in r.stdout, r.stdout + r.stderr
