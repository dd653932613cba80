"""CPU: the surface of the attention roll-out -- the C-ABI declaration of i2r_attn_rollout_step, the plan / layout / validation of
attn_capture.RolloutForm, the ValueErrors of net.rollout_at / net.person_rollout that need no engine, the identities of the float64
reference (tests/_attn_rollout_ref.py), and the CONDITION on the inputs of the raw GPU cases: the same chain taken by torch in float32 on
the CPU stays within a quarter of the bar (steps x 1e-5) of the float64 product, for every raw case of tests/test_attn_rollout_gpu.py --
the reference arithmetic alone, so a GPU miss of the bar is the kernel's."""
import ctypes
import os
import re

import pytest
import torch

import _attn_rollout_ref as ref
from i2r_amd import attn_capture, cabi, config, models
from i2r_amd.attn_capture import Rollout, RolloutForm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LAYERS = 6


def test_header_declares_attn_rollout_step():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert re.search(r"^I2R_API int i2r_attn_rollout_step\(const i2r_attn_rollout_args\* a, void\* stream\);", header, flags=re.M)
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == cabi.ABI_VERSION == 17  # additive
    assert "i2r_attn_rollout_step" in cabi.EXPORTS
    fields = re.search(r"typedef struct i2r_attn_rollout_args \{(.*?)\} i2r_attn_rollout_args;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f.rstrip("_") for f, _ in cabi.AttnRolloutArgs._fields_]
    n_ptr = sum(1 for _, t in cabi.AttnRolloutArgs._fields_ if t is cabi._fp)
    assert n_ptr == 10 and all(t is cabi._fp for _, t in cabi.AttnRolloutArgs._fields_[:n_ptr])  # pointers first: no padding holes
    assert dict(cabi.AttnRolloutArgs._fields_)["alpha"] is ctypes.c_float
    assert ctypes.sizeof(cabi.AttnRolloutArgs) == 8 * n_ptr + 4 * (len(names) - n_ptr) == 136
    for text in ("A_l = (1 - alpha) I + alpha P_l", "T   = A_hi A_hi-1 ... A_lo"):  # the definitions, verbatim
        assert text in header and text in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_built_library_exports_attn_rollout_step():
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert L.i2r_attn_rollout_step.argtypes[0]._type_ is cabi.AttnRolloutArgs
    assert L.i2r_attn_rollout_step(None, None) == -1 and b"null pointer" in L.i2r_last_error()  # (rejected on the host: no GPU needed)
    a = cabi.AttnRolloutArgs()
    for f in ("qk", "in_", "out", "grp_off", "x_off", "ws", "grp_off_host"):
        setattr(a, f, 4096)
    a.alpha = 0.5
    assert L.i2r_attn_rollout_step(ctypes.byref(a), None) == -1 and b"in == out" in L.i2r_last_error()
    a.out, a.side = 8192, 2
    assert L.i2r_attn_rollout_step(ctypes.byref(a), None) == -1 and b"side=2" in L.i2r_last_error()
    a.side, a.alpha = 1, 1.25
    assert L.i2r_attn_rollout_step(ctypes.byref(a), None) == -1 and b"alpha=1.25" in L.i2r_last_error()


# ---- the form ------------------------------------------------------------------------------------------------------------------------
def test_rollout_call_object():
    r = Rollout({"s": torch.zeros(2, 5, dtype=torch.int32)}, "affect", 0.25, {"s": 4})
    assert (r.points, r.mode, r.alpha, r.capacity, r.upsample) == (True, 1, 0.25, 5, {"s": 4})
    p = Rollout(None, "affect", 1.0, 2)
    assert (p.points, p.mode, p.capacity) == (False, 2, 0) and Rollout(None, None).mode == 0 and Rollout(None).mode == 1
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            Rollout(None, None, bad)
    for tokens, bad in (({"s": [[0]]}, None), ({"s": [[0]]}, "rows"), (None, "rows"), (None, True), ({"s": [[0]]}, 2)):
        with pytest.raises(ValueError, match="mode"):
            Rollout(tokens, bad)


def test_form_key_layers_and_sides():
    cap = {("a", 1), ("a", 2), ("a", 3), ("b", 0)}
    tok = {"a": torch.zeros(2, 3, dtype=torch.int32), "b": torch.zeros(1, 3, dtype=torch.int32)}
    f = RolloutForm(cap, Rollout(tok, "affect", 0.5, {"a": 4, "b": 16}))
    assert f.deferred and f.per_stack and not f.merged and f.N_BLOCKS == 2 and f.side == 1
    assert f.range == {"a": (1, 3), "b": (0, 0)}
    assert f.key == ("capture", cap, "rollout", "points", 1, 3, (("a", 4), ("b", 16)))
    # alpha, the points and the counts are per call: the key is the same
    assert RolloutForm(cap, Rollout({k: v + 1 for k, v in tok.items()}, "affect", 0.9, {"a": 4, "b": 16}, counts={"a": [1, 2]})).key == f.key
    assert RolloutForm(cap, Rollout(tok, "dependency", 0.5, {"a": 4, "b": 16})).key != f.key
    with pytest.raises(ValueError, match="contiguous"):
        RolloutForm({("a", 0), ("a", 2)}, Rollout({"a": tok["a"]}))
    with pytest.raises(ValueError, match="no table"):
        RolloutForm(cap, Rollout({"a": tok["a"]}))
    with pytest.raises(ValueError, match="no scale"):
        RolloutForm(cap, Rollout(tok, upsample={"a": 2}))
    with pytest.raises(ValueError, match="upsample"):
        RolloutForm(cap, Rollout(tok, upsample=65))
    sides = [RolloutForm(frozenset({("i", 0)}), Rollout(None, m)) for m in (None, "dependency", "affect")]
    assert [(s.N_BLOCKS, s.mode, s.side) for s in sides] == [(3, 0, 0), (3, 1, 0), (3, 2, 1)]
    assert len({s.key for s in sides}) == 3 and sides[0].key[2:4] == ("rollout", "persons")


def test_plan_at_query_tokens():
    tok = torch.tensor([[0, 5, -1], [3, 3, 1]], dtype=torch.int32)
    f = RolloutForm({("s", 0), ("s", 1), ("s", 2)}, Rollout({"s": tok}, "affect", 0.5, 2, {"s": [3, 2]}))
    p = f.plan("s", (2, 3), [12, 6], 2, f.call)
    maps, xl = p.blocks
    assert maps.shapes == [(3, 2, 4, 6), (2, 1, 4, 6)] and maps.offs == [0, 144, 192] and maps.base == 0 and p.layer_floats == 192
    assert xl.shapes is None and xl.offs == [0, 36, 48] and xl.base == p.layer_floats  # the working matrices: behind the blocks
    assert p.extra_floats == 2 * 48 and p.K == 3 and p.rows_floats == 3 * 18 and p.n_grp == 2
    assert p.ws_stride == 2 * 2 * 1 and p.ws_floats == p.ws_stride * 18
    assert [t.tolist() for t in p.tables] == [[3, 2]]
    idx, value = p.seed
    assert idx.tolist() == [0, 12 + 5, 36 + 3, 36 + 6 + 3] and value == 1.0 and idx.dtype == torch.int64  # (the -1 entry: a zero row)
    X = torch.zeros(48).index_fill_(0, idx, value)
    assert torch.equal(X[:36].view(3, 12), ref.seed_points(tok[0], 12, torch.float32))
    assert torch.equal(X[36:].view(2, 6), ref.seed_points(tok[1, :2], 6, torch.float32))
    assert f.plan("s", (2, 3), [12, 6], 2, Rollout({"s": tok}, "affect", 0.5, 1)).rows_floats == 54  # (the form's scale, not the call's)
    f1 = RolloutForm({("s", 0)}, Rollout({"s": tok}))
    assert f1.plan("s", (2, 3), [12, 6], 1, f1.call).rows_floats == 1
    for bad, msg in ((torch.tensor([[0, 12, 0], [0, 0, 0]]), "outside"), (torch.zeros(3, 3), "shape"), (torch.zeros(2, 0), "shape")):
        with pytest.raises(ValueError, match=msg):
            f.plan("s", (2, 3), [12, 6], 2, Rollout({"s": bad}, "affect"))
    with pytest.raises(ValueError, match="counts"):
        f.plan("s", (2, 3), [12, 6], 2, Rollout({"s": tok}, "affect", counts={"s": [4, 1]}))


@pytest.mark.parametrize("mode,side,value", [(None, 0, 1 / 6), ("dependency", 0, 1 / 6), ("affect", 1, 1.0)])
def test_plan_per_person(mode, side, value):
    f = RolloutForm({("s", 0), ("s", 1)}, Rollout(None, mode, 0.5, 2))
    p = f.plan("s", (2, 3), [12, 6], 2, f.call)
    rel, maps, xl = p.blocks
    assert rel.shapes == [(2, 2), (1, 1)] and rel.offs == [0, 4, 5] and rel.base == 0
    assert maps.shapes == (None if mode is None else [(2, 2, 4, 6), (1, 1, 4, 6)]) and maps.base == 8
    assert xl.offs == [0, 24, 30] and xl.shapes is None and xl.base == p.layer_floats == (8 if mode is None else 128)
    assert p.K == 2 and p.tables == () and p.extra_floats == 64 and p.rows_floats == 2 * 18
    idx, v = p.seed
    assert v == value
    X = torch.zeros(32, dtype=torch.float64).index_fill_(0, idx, v)
    assert torch.equal(X[:24].view(2, 12), ref.seed_persons(2, 6, side)) and torch.equal(X[24:30].view(1, 6), ref.seed_persons(1, 6, side))
    views = [{("s", 0): "R"}, {("s", 0): "M"} if mode else {}, {}]
    assert f.result(views, None) == ({"s": "R"}, {"s": "M"} if mode else {})


def test_resolve_serves_and_refuses():
    stacks, inter = {"singleformer.global_encoder": 3, "global_encoder": 2}, "global_encoder"
    cap = {(inter, 0), (inter, 1)}
    pts = Rollout({inter: torch.zeros(1, 2, dtype=torch.int32)})
    res = lambda **kw: attn_capture.resolve(**{**dict(capture=cap, queries=None, persons=None, flip_joint_map=None, stacks=stacks, inter_stack=inter,  # noqa: E731
                                                      window=False, rollout=pts), **kw})
    assert isinstance(res(), RolloutForm) and isinstance(res(rollout=Rollout(None)), RolloutForm)
    assert list(attn_capture.resolve.__code__.co_varnames[:attn_capture.resolve.__code__.co_argcount])[-1] == "rollout"  # the new parameter goes last
    assert attn_capture.resolve.__defaults__[-1] is None
    for kw, msg in ((dict(window=True), "window"), (dict(flip_joint_map=object()), "flip test"), (dict(flip_joint_map=object(), flip_maps="merged"), "flip test"),
                    (dict(queries=object()), "queries="), (dict(persons=object()), "persons="), (dict(joints=object()), "predicted-joint"),
                    (dict(capture=None), "needs capture"), (dict(capture={(inter, 2)}), "encoder stacks"), (dict(capture={("x", 0)}), "encoder stacks"),
                    (dict(capture={(inter, 0), ("singleformer.global_encoder", 0)}, rollout=Rollout(None)), "inter-human stack"),
                    (dict(capture={("singleformer.global_encoder", 0), ("singleformer.global_encoder", 2)},
                          rollout=Rollout({"singleformer.global_encoder": torch.zeros(1, 1)})), "contiguous")):
        with pytest.raises(ValueError, match=msg):
            res(**kw)
    # the forms that were there resolve as before
    assert isinstance(res(rollout=None), attn_capture.FullForm) and res(rollout=None, capture=None) is None


def test_public_calls_refuse_what_is_not_served():
    x, m = torch.zeros(1, 3, 256, 192), torch.zeros(1, 1, 256, 192)
    pts = torch.zeros(1, 2, 2)
    cfg = config.load_config("tph_192_p6_b4")
    alone = [models.transpose_h.get_pose_net(cfg, is_train=False), models.hrformer.get_pose_net(config.load_config("hrt_192_p4_b4"), is_train=False)]
    for net in alone:  # the stand-alone first-stage models
        with pytest.raises(ValueError, match="stand-alone"):
            net.rollout_at(x, m, [1], pts)
        with pytest.raises(ValueError, match="stand-alone"):
            net.person_rollout(x, m, [1])
    win = models.interformer.get_pose_net(config.load_config("tph_192_p6_b4", ["MODEL.ATTENTION_TYPE", "window", "MODEL.N_HEAD", 4]), is_train=False)
    with pytest.raises(ValueError, match="ATTENTION_TYPE"):
        win.rollout_at(x, m, [1], pts)
    with pytest.raises(ValueError, match="ATTENTION_TYPE"):
        win.person_rollout(x, m, [1])
    net = models.interformer.get_pose_net(cfg, is_train=False)
    with pytest.raises(ValueError, match="flip_pairs"):
        net.rollout_at(x, m, [1], pts, flip_pairs=[[1, 2]])
    with pytest.raises(ValueError, match="flip_pairs"):
        net.person_rollout(x, m, [1], flip_pairs=[[1, 2]])
    for joints in (None, "joints"):  # predicted-joint queries
        with pytest.raises(ValueError, match="predicted-joint"):
            net.rollout_at(x, m, [1], joints)
    with pytest.raises(ValueError, match="maps"):
        net.person_rollout(x, m, [1], maps="rows")
    with pytest.raises(ValueError, match="rollout="):  # the grouped forward (refused before anything touches a device)
        net.forward_main_target(x, m, [1], torch.zeros(1, 2), max_patch=2, rollout=Rollout(None))
    have = {"a": 6, "b": 2}
    cap = net._rollout_capture
    assert cap(have, "t", None, None) == {("a", i) for i in range(6)} | {("b", 0), ("b", 1)}
    assert cap(have, "t", ["a"], (2, 4)) == {("a", 2), ("a", 3), ("a", 4)} == cap(have, "t", "a", {"a": (2, 4)})
    assert cap(have, "t", None, {("a", 0), ("a", 2)}) == {("a", 0), ("a", 2)}  # (a hole: RolloutForm refuses it)
    for stacks, layers in ((["c"], None), (None, {"a": (3, 6)}), (None, {"a": (2, 1)}), (["b"], (0, 2)), (None, {"c": (0, 0)})):
        with pytest.raises(ValueError):
            cap(have, "t", stacks, layers)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,pers", [(1, 4), (12, 3), (48, 2)])
def test_reference_identities(seg, pers):
    L = pers * seg
    maps = [ref.full_map(ref.make_qk(2, 16, L, 10 * seg + l)[0], 2, 16, 48) for l in range(3)]
    for alpha in (0.0, 0.5, 1.0):
        T = ref.rollout(maps, alpha)
        assert (T.sum(1) - 1).abs().max().item() < 1e-12  # T 1 = 1
        D, F, R, R2 = ref.reduce_persons(T, seg)
        assert (R - R2).abs().max().item() < 1e-12  # R_T = sum_{k in j} D_T = mean_{q in i} F_T
        assert (D.sum(1) - 1).abs().max().item() < 1e-12 and (F.sum(0) - 1).abs().max().item() < 1e-12
        for side, want in ((0, D), (1, F)):  # the thin chains ARE the reductions of T
            X = ref.chain(ref.seed_persons(pers, seg, side), maps, alpha, side)
            assert (X - want).abs().max().item() < 1e-12 and (ref.relation_from(X, seg, side) - R).abs().max().item() < 1e-12
        tok = torch.tensor([L - 1, -1, 0])
        for side in (0, 1):
            assert (ref.chain(ref.seed_points(tok, L), maps, alpha, side) - ref.at_tokens(T, tok, side)).abs().max().item() < 1e-12
        if alpha == 0.0:
            assert torch.equal(T, torch.eye(L, dtype=torch.float64))
        if alpha == 1.0:
            assert (T - maps[2] @ maps[1] @ maps[0]).abs().max().item() < 1e-12


def _float32_condition(lens, offs, heads, hp, case, seeds_of):
    """for every chain of the GPU test on these groups: the float32 chain on the CPU against the float64 T, within a quarter of the bar"""
    n_tok = offs[-1] + lens[-1] + 24
    qk = [ref.make_qk(heads, hp, n_tok, ref.layer_seed(heads, hp, case, l)) for l in range(N_LAYERS)]
    k_off = qk[0][1]
    worst = 0.0
    for g, (o, n) in enumerate(zip(offs, lens)):
        if n == 0:
            continue
        m64 = [ref.full_map(q[o:o + n], heads, hp, k_off) for q, _, _ in qk]
        m32 = [ref.map_of(q[o:o + n], heads, hp, k_off, torch.float32) for q, _, _ in qk]
        for steps, alpha in ref.CHAINS:
            T = ref.rollout(m64[:steps], alpha)
            for side in (0, 1):
                for seed, want in seeds_of(g, n, side, T):
                    got = ref.chain(seed, m32[:steps], alpha, side)
                    assert got.dtype == torch.float32
                    e = (got.double() - want).abs().max().item()
                    worst = max(worst, e / steps)
                    assert e <= steps * ref.BAR / 4, "heads=%d hp=%d group %d side %d, %d steps alpha %g: float32 chain %.2e" % (heads, hp, g, side, steps, alpha, e)
    return worst


@pytest.mark.parametrize("heads,hp", ref.HEADS_HP)
def test_float32_chain_meets_a_quarter_of_the_bar_on_every_raw_case(heads, hp):
    offs = [ref.QUERY_START]
    for n in ref.QUERY_LENS[:-1]:
        offs.append(offs[-1] + n)

    def at_points(g, n, side, T):
        for K, cnt in ref.QUERY_K:
            tok = ref.query_tokens(K, ref.QUERY_LENS, 31 * K + heads)[g, :(cnt or [K] * len(ref.QUERY_LENS))[g]]
            yield ref.seed_points(tok, n, torch.float32), ref.at_tokens(T, tok, side)

    worst = [_float32_condition(ref.QUERY_LENS, offs, heads, hp, 0, at_points)]
    for ci, (seg, pers, start) in enumerate(ref.PERSON_CASES):
        lens = [p * seg for p in pers]
        offs = [start]
        for n in lens[:-1]:
            offs.append(offs[-1] + n)

        def per_person(g, n, side, T, seg=seg):
            yield ref.seed_persons(n // seg, seg, side, torch.float32), ref.reduce_persons(T, seg)[side]

        worst.append(_float32_condition(lens, offs, heads, hp, 1 + ci, per_person))
    print("heads=%d hp=%d: float32 chain on the CPU, worst max-abs per step %.2e (a quarter of the bar: 2.5e-6)" % (heads, hp, max(worst)))
