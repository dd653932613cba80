"""CPU: the surface of the attention maps under the flip test -- the C-ABI declarations of i2r_attn_flip_merge and i2r_token_mirror, the
mirror mu, the identities of the float64 reference (tests/_attn_flip_ref.py), the plan and the program key of a merged form, and the
errors that need no engine."""
import ctypes
import dataclasses
import os
import re

import pytest
import torch

from _attn_flip_ref import as_query_maps, merged_map, merged_persons, merged_query_maps, mirror_tokens, unmirror_map
from _attn_person_ref import full_map, reduce_persons
from _attn_query_ref import query_maps
from i2r_amd import cabi, config, models
from i2r_amd.attn_capture import AttnQueries, JointForm, JointQueries, PersonForm, PersonMaps, QueryForm, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_struct_layout_agree():
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == cabi.ABI_VERSION == 17
    assert re.search(r"^I2R_API int i2r_attn_flip_merge\(const i2r_attn_flip_merge_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"^I2R_API int i2r_token_mirror\(const int32_t\* src, int32_t\* dst, int64_t n, int32_t w, void\* stream\);", header, flags=re.M)
    assert "i2r_attn_flip_merge" in cabi.EXPORTS and "i2r_token_mirror" in cabi.EXPORTS
    fields = re.search(r"typedef struct i2r_attn_flip_merge_args \{(.*?)\} i2r_attn_flip_merge_args;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f for f, _ in cabi.AttnFlipMergeArgs._fields_]
    n_ptr = sum(1 for _, t in cabi.AttnFlipMergeArgs._fields_ if t is cabi._fp)
    assert n_ptr == 8 and names[:n_ptr] == [f for f, t in cabi.AttnFlipMergeArgs._fields_ if t is cabi._fp]  # pointers first: no padding holes
    assert all(t is cabi._i32 for _, t in cabi.AttnFlipMergeArgs._fields_[n_ptr:])
    assert ctypes.sizeof(cabi.AttnFlipMergeArgs) == 8 * n_ptr + 4 * (len(names) - n_ptr) == 88  # 8 pointers, 6 int32
    # no existing struct changed
    assert (ctypes.sizeof(cabi.AttnQueryArgs), ctypes.sizeof(cabi.AttnPersonArgs), ctypes.sizeof(cabi.AttnWeightsArgs)) == (128, 120, 72)


def test_built_library_exports_the_entries_and_rejects_on_the_host():
    L = cabi.load_library()
    assert L.i2r_abi_version() == 17
    assert L.i2r_attn_flip_merge.argtypes[0]._type_ is cabi.AttnFlipMergeArgs
    assert L.i2r_attn_flip_merge(None, None) == -1 and b"null pointer" in L.i2r_last_error()  # (rejected on the host: no GPU needed)
    assert L.i2r_attn_flip_merge(ctypes.byref(cabi.AttnFlipMergeArgs()), None) == -1 and b"null pointer" in L.i2r_last_error()
    assert L.i2r_token_mirror(None, None, 4, 3, None) == -1 and b"null pointer" in L.i2r_last_error()
    host_off = (ctypes.c_int32 * 3)(0, 10, 30)

    def args(**kw):  # (pointers that nothing dereferences on the host; every call below is rejected before a launch)
        d = dict(a=64, b=64, out=64, grp_off=64, src_off=64, out_off=64, grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=2, K=3, seg=0,
                 scale=1, h=5, w=2)
        d.update(kw)
        return cabi.AttnFlipMergeArgs(**d)

    for ptr in ("a", "b", "out", "grp_off", "src_off", "out_off", "grp_off_host"):
        assert L.i2r_attn_flip_merge(ctypes.byref(args(**{ptr: None})), None) == -1 and b"null pointer" in L.i2r_last_error(), ptr
    for kw, msg in ((dict(scale=0), b"scale=0"), (dict(scale=65), b"scale=65"), (dict(h=0), b"h=0"), (dict(w=0), b"w=0"), (dict(h=3, w=1), b"not a multiple"),
                    (dict(h=2, w=2), b"not a multiple"), (dict(seg=4), b"not a multiple"), (dict(seg=-1), b"seg=-1"), (dict(K=0), b"K=0"),
                    (dict(n_grp=0), b"n_grp=0"), (dict(n_grp=65536), b"n_grp=65536")):
        assert L.i2r_attn_flip_merge(ctypes.byref(args(**kw)), None) == -1, kw
        assert msg in L.i2r_last_error(), (kw, L.i2r_last_error())
    for bad in ((64, 64, -1, 3), (64, 64, 4, 0), (None, 64, 4, 3), (64, None, 4, 3)):
        assert L.i2r_token_mirror(*bad, None) == -1, bad


@pytest.mark.parametrize("w", [1, 2, 5, 12])
def test_mu_is_an_involution_and_keeps_negatives(w):
    h, P = 3, 2
    t = torch.arange(P * h * w)
    mu = mirror_tokens(t, w)
    assert torch.equal(mirror_tokens(mu, w), t) and sorted(mu.tolist()) == t.tolist()
    p, y, x = t // (h * w), t // w % h, t % w
    assert torch.equal(mu, p * h * w + y * w + (w - 1 - x))  # mu(p, y, x) = (p, y, w - 1 - x)
    if w % 2:
        assert torch.equal(mu[x == w // 2], t[x == w // 2])  # the centre column maps to itself
    neg = torch.tensor([-1, 0, -7, w - 1, -(2 ** 31)])
    got = mirror_tokens(neg, w)
    assert got[[0, 2, 4]].tolist() == [-1, -7, -(2 ** 31)] and got[[1, 3]].tolist() == [w - 1, 0]


def _two_passes(P, h, w, heads, hp, seed):
    g = torch.Generator().manual_seed(seed)
    L = P * h * w
    return [full_map(torch.randn(L, 2 * heads * hp + 8, generator=g, dtype=torch.float64), heads, hp, heads * hp + 8) for _ in range(2)]


@pytest.mark.parametrize("P,h,w", [(1, 1, 1), (1, 3, 1), (2, 3, 5), (3, 4, 6)])
def test_reference_identities(P, h, w):
    full, full_m = _two_passes(P, h, w, 2, 16, 10 * P + w)
    L, T = P * h * w, h * w
    M = merged_map(full, full_m, w)
    assert (M.sum(1) - 1).abs().max().item() < 1e-12, "merged dependency rows sum to 1"
    assert (unmirror_map(unmirror_map(full_m, w), w) - full_m).abs().max().item() == 0
    if w == 1:
        assert torch.equal(M, (full + full_m) / 2)
    D, F, R = merged_persons(full, full_m, h, w)
    assert (F.sum(0) - 1).abs().max().item() < 1e-12, "sum_j F_m = 1"
    assert (R.sum(1) - 1).abs().max().item() < 1e-12, "rows of R_m sum to 1"
    assert (D.sum(1) - 1).abs().max().item() < 1e-12
    assert (R - D.reshape(P, P, T).sum(2)).abs().max().item() < 1e-12, "R_m[i, j] = sum_{k in j} D_m[i, k]"
    assert (R - F.reshape(P, P, T).mean(2).t()).abs().max().item() < 1e-12
    # the decomposition is the reduction of the merged map: sums over whole persons are mirror-invariant
    D2, F2, R2, _ = reduce_persons(M, T)
    assert max((D - D2).abs().max().item(), (F - F2).abs().max().item(), (R - R2).abs().max().item()) < 1e-12
    # the query form's decomposition gives the rows / columns of the merged map
    tok = torch.tensor([0, L - 1, -1, L // 2, L // 2])
    for mode in (0, 1):
        got = merged_query_maps(full, full_m, tok, mode, h, w)
        assert (got - query_maps(M, tok, mode, h, w)).abs().max().item() < 1e-12
        assert not got[2].any(), "a skipped entry is a zero map"
        up = merged_query_maps(full, full_m, tok, mode, h, w, 2)
        assert up.shape == (5, P, 2 * h, 2 * w) and (up - query_maps(M, tok, mode, h, w, 2)).abs().max().item() < 1e-12
    assert torch.equal(as_query_maps(M[:1], h, w), M[:1].reshape(1, P, h, w))


def _ints_only(p):
    """a plan holds integers (and lists / tuples / Blocks of them); its tables are host int32 tensors or shapes"""
    def ok(v):
        if v is None or (isinstance(v, int) and not isinstance(v, bool)):
            return True
        return isinstance(v, (list, tuple)) and all(ok(e) for e in v)
    for f in dataclasses.fields(p):
        v = getattr(p, f.name)
        if f.name == "tables":
            assert all((torch.is_tensor(t) and t.device.type == "cpu" and t.dtype == torch.int32) or ok(t) for t in v)
        else:
            assert ok(v), (f.name, v)


def test_plan_of_a_merged_form_holds_integers_only():
    st, cap = "enc", frozenset({("enc", 0), ("enc", 1)})
    lens, cnt = [24, 12], [5, 3]
    tok = torch.tensor([[0, 23, -1, 5, 5], [1, 11, 2, -1, -1]], dtype=torch.int32)
    q = AttnQueries({st: tok}, "dependency", 2, {st: cnt})
    plain, merged = QueryForm(cap, q), QueryForm(cap, q).merge()
    p0, p1 = plain.plan(st, (3, 4), lens, 2, q), merged.plan(st, (3, 4), lens, 2, q)
    _ints_only(p0)
    _ints_only(p1)
    assert (p0.raw_offs, p0.raw_floats) == ((), 0) and (p1.raw_offs, p1.raw_floats) == ((0, 120), 156)  # 5 x 24, then 3 x 12
    assert p1.rows_floats == 1 and p0.rows_floats == 5 * 36  # the merged form's launches run at scale 1: no rows workspace
    assert (p1.blocks, p1.layer_floats, p1.n_tiles, p1.ws_floats) == (p0.blocks, p0.layer_floats, p0.n_tiles, p0.ws_floats)
    for mode, raw in ((0, ((), 0)), (1, ((0, 108), 120)), (2, ((0, 108), 120))):  # images of 3 and 1 persons: 3 x 36, then 1 x 12
        p = PersonForm(cap, PersonMaps(mode, 2)).merge().plan(st, (3, 4), [36, 12], 2)
        _ints_only(p)
        assert (p.raw_offs, p.raw_floats) == raw and p.rows_floats == 3 * 48
        assert p.blocks == PersonForm(cap, PersonMaps(mode, 2)).plan(st, (3, 4), [36, 12], 2).blocks
    j = JointForm(cap, JointQueries("affect", 4), 17).merge()
    p = j.plan(st, (3, 4), [36, 12], 2)
    _ints_only(p)
    assert p.raw_offs == (0, 51 * 36) and p.raw_floats == 51 * 36 + 17 * 12 and p.tables[0] == (2, 51)


def test_program_keys():
    stacks = {"single": 4, "inter": 6}
    args = (stacks, "inter", False)
    cap = {("inter", 0), ("single", 3)}
    q = AttnQueries({"inter": torch.zeros(2, 7), "single": torch.zeros(4, 3)}, "affect", {"inter": 16, "single": 4}, capacity=9)
    # the un-flipped keys are what they were
    kq = ("capture", frozenset(cap), "query", 1, 9, (("inter", 16), ("single", 4)))
    kp = ("capture", frozenset({("inter", 5)}), "persons", 2, 16)
    kj = ("capture", frozenset(cap), "query", 0, 17, (("inter", 1), ("single", 1)), "joints")
    assert resolve(cap, q, None, None, *args).key == kq and resolve(cap, q, None, None, *args, flip_maps="plain").key == kq
    assert resolve({("inter", 5)}, None, PersonMaps("affect", 16), None, *args).key == kp
    assert resolve(cap, None, None, None, *args, JointQueries(), 17).key == kj
    f = resolve(cap, None, None, "flip", *args, JointQueries(), 17)  # the plain pass's maps under the flip test: as before
    assert f.key == kj and f.deferred and not f.merged
    # the merged forms: the same keys plus the marker, all deferred
    for a, key in (((cap, q, None), kq), (({("inter", 5)}, None, PersonMaps("affect", 16)), kp)):
        f = resolve(*a, "flip", *args, flip_maps="merged")
        assert f.key == key + ("flip-merged",) and f.merged and f.deferred
        assert not resolve(*a, None, *args).deferred
    f = resolve(cap, None, None, "flip", *args, JointQueries(), 17, flip_maps="merged")
    assert type(f) is JointForm and f.key == kj + ("flip-merged",) and f.merged and f.deferred
    # what stays refused
    for bad, match in (((cap, q, None, None), "needs the flip test"), ((cap, None, None, "flip"), "exactly one of"),
                       (({("inter", 0)}, q, PersonMaps(), "flip"), "exactly one of"), ((None, q, None, "flip"), "needs capture")):
        with pytest.raises(ValueError, match=match):
            resolve(*bad, *args, flip_maps="merged")
    with pytest.raises(ValueError, match="ATTENTION_TYPE window"):
        resolve(cap, q, None, "flip", stacks, "inter", True, flip_maps="merged")
    with pytest.raises(ValueError, match="flip_maps"):
        resolve(cap, q, None, None, *args, flip_maps="both")
    with pytest.raises(ValueError, match="not with"):  # the per-person form under the flip test without the choice: as before
        resolve({("inter", 0)}, None, PersonMaps(), "flip", *args)
    with pytest.raises(AssertionError):
        resolve(cap, q, None, "flip", *args)


def test_module_calls_check_flip_maps_without_an_engine():
    net = models.interformer.get_pose_net(config.load_config("tph_192_p6_b4"), is_train=False)
    assert net._flip_map(None, None, "merged", "attention_at", "merged") == (None, "plain")
    with pytest.raises(ValueError, match="flip_maps"):
        net._flip_map(None, None, "both", "attention_at", "merged")
    with pytest.raises(ValueError, match="only flip_maps='merged'"):
        net._flip_map(None, [[1, 2]], "plain", "person_relations", "merged")
