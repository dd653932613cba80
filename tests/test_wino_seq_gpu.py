"""-m gpu: Winograd workgroups that run several fragments on one set-up (i2r_conv_desc.seq, csrc/i2r_conv_wino.hip).  Every launch is
checked two ways: bit for bit against the same launch at seq = 1, and against float64 at the bar of
tests/test_kernels_gpu.py::test_conv_winograd_matches_torch_and_direct (2e-5 of max |ref|)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _conv_cases as cc
from _golden import setup
from _gpu_util import from_act, run, to_act
from i2r_amd import cabi, engine, models, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEQS = (2, 3, 4)


def _rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(23, key, tuple(shape), scale))


class Member:
    """one conv of a launch: input (with up-sampled terms at 1 / scales: the fused-input form), folded BN, residual before / after the ReLU"""

    def __init__(self, n, cin, cout, h, w, tag, scales=(), res1=False, res_post=False, relu=True):
        self.scales, self.tag, self.relu = scales, tag, relu
        self.sd = {"c.weight": _rand((cout, cin, 3, 3), "w" + tag, (6.0 / (cin * 9)) ** 0.5),
                   "b.weight": _rand((cout,), "g" + tag, 0.5) + 1.0, "b.bias": _rand((cout,), "b" + tag, 0.3),
                   "b.running_mean": _rand((cout,), "m" + tag, 0.3), "b.running_var": _rand((cout,), "v" + tag, 0.4) + 1.0}
        self.base = _rand((n, cin, h, w), "x" + tag)
        self.terms = [_rand((n, cin, h // s, w // s), "t%d%s" % (s, tag)) for s in scales]
        self.res1 = _rand((n, cout, h, w), "r1" + tag) if res1 else None
        self.res_post = _rand((n, cout, h, w), "rp" + tag) if res_post else None
        y = self.base.double()
        for t, s in zip(self.terms, scales):
            y = y + F.interpolate(t.double(), scale_factor=s, mode="nearest")
        y = F.relu(y) if scales else y
        sd = {k: v.double() for k, v in self.sd.items()}
        ref = F.batch_norm(F.conv2d(y, sd["c.weight"], None, padding=1), sd["b.running_mean"], sd["b.running_var"], sd["b.weight"], sd["b.bias"], False, 0.0, 1e-5)
        if res1:
            ref = ref + self.res1.double()
        if relu:
            ref = F.relu(ref)
        if res_post:
            ref = ref + self.res_post.double()
        self.ref = ref

    def emit(self, P, grp, fused=True):
        pc = engine.Packer(self.sd, torch.device(DEV)).conv("c", "b")
        base, terms = to_act(P, self.base), [to_act(P, t) for t in self.terms]
        kw = dict(relu=self.relu, group=grp, res1=to_act(P, self.res1) if self.res1 is not None else None,
                  res_post=to_act(P, self.res_post) if self.res_post is not None else None)
        self.y = None
        if not self.scales:
            self.out = P.conv(base, pc, **kw)
            return
        self.y = P.alloc(base.n, base.h, base.w, base.c)
        self.y.t.fill_(float("nan"))
        if fused:
            self.out = P.conv(base, pc, fuse_in=(terms, self.y), **kw)
        else:
            P.fuse_up_add(base, terms, self.y, relu=True)
            self.out = P.conv(self.y, pc, **kw)


def _counts(d, seq):
    """(runs, channel blocks) of a member at run length seq"""
    nfrag = d.n_img * -(-d.conv_h // d.tile_h) * -(-d.conv_w // d.tile_w)
    n_cblk = (d.cout_pad // 16) // (3 if (d.cout_pad // 16) % 3 == 0 else 4)
    return -(-nfrag // seq), n_cblk


def _launch(ms, seqs, table=False, fused=True):
    """-> [(y or None, out as stored, out NCHW float64)] per member, of ONE grouped launch with the members' seq forced"""
    dev = torch.device(DEV)
    P = engine.Program(dev)
    grp = []
    for m in ms:
        m.emit(P, grp, fused)
    descs = [g[0] for g in grp]
    for d, s in zip(descs, seqs):
        assert d.algo == 1
        d.seq = s
    P.flush_group(grp)
    (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
    slots = [st.d[i].contents for i in range(st.n)]
    # the grid the library reports = the run counts, with a table and in whole rounds of 8 runs per member without
    arr = (C.POINTER(cabi.ConvDesc) * st.n)(*[st.d[i] for i in range(st.n)])
    for with_map in (1, 0):
        g, got_seq = C.c_int32(-1), (C.c_int32 * st.n)()
        cabi.check(cabi.lib().i2r_conv_grid(arr, st.n, with_map, C.byref(g), got_seq), "i2r_conv_grid")
        want = [_counts(d, d.seq) for d in slots]
        assert list(got_seq) == [d.seq for d in slots]
        assert g.value == sum(r * c if with_map else -(-r // 8) * 8 * c for r, c in want), (g.value, want, with_map)
    if table:  # the members interleaved, each walking its runs backwards (entry = member << 24 | run * channel blocks + block)
        left = [r * c for r, c in (_counts(d, d.seq) for d in slots)]
        order = []
        while any(left):
            for i in range(st.n):
                if left[i]:
                    left[i] -= 1
                    order.append((i << 24) | left[i])
        bm = torch.tensor(order, dtype=torch.int32, device=dev)
        P.keep.append(bm)
        st.block_map, st.map_len = bm.data_ptr(), bm.numel()
    run(P)
    return [(m.y.view().clone() if m.y is not None else None, m.out.view().clone(), from_act(m.out).double()) for m in ms]


def _check(ms, base, got, what):
    for m, (y1, o1, _), (y, o, o64) in zip(ms, base, got):
        assert torch.equal(o, o1), "%s %s: out differs from seq 1, max |d| %.3e" % (what, m.tag, (o - o1).abs().max().item())
        if y1 is not None:
            assert not torch.isnan(y).any(), "%s %s: y not written completely" % (what, m.tag)
            assert torch.equal(y, y1), "%s %s: y differs from seq 1" % (what, m.tag)
        err, bar = (o64 - m.ref).abs().max().item(), 2e-5 * m.ref.abs().max().item()
        print("%s %s: max |got - ref| %.3e (bar %.3e)" % (what, m.tag, err, bar))
        assert err < bar, "%s %s: max-abs %.3e, bar %.3e" % (what, m.tag, err, bar)


SINGLE = {
    "straddle-empty-tail": lambda: [Member(3, 48, 48, 16, 12, "st")],            # 3 fragments per crop, 9 in all
    "res1-two-blocks": lambda: [Member(2, 48, 96, 32, 24, "rb", res1=True)],
    "one-pass-res-post": lambda: [Member(1, 16, 48, 64, 48, "op", res_post=True)],
    "ragged-map": lambda: [Member(1, 48, 48, 18, 10, "rg")],                      # the map is no multiple of the fragment
    "nt4": lambda: [Member(2, 64, 64, 16, 12, "n4")],                             # conv_wino_f32<1, 4>
    "fused-input": lambda: [Member(2, 48, 48, 32, 24, "f48", scales=(2, 4)), Member(2, 96, 96, 32, 24, "f96", scales=(2, 4))],
}
_BASE = {}  # case -> (members with their float64 references, results at seq 1): computed once, shared by the seq cases


def _base(name, make, **kw):
    if name not in _BASE:
        ms = make()
        _BASE[name] = (ms, _launch(ms, [1] * len(ms), **kw))
        _check(ms, _BASE[name][1], _BASE[name][1], name + " seq 1")
    return _BASE[name]


@pytest.mark.parametrize("seq", SEQS)
@pytest.mark.parametrize("name", list(SINGLE))
def test_runs_of_fragments_match_one_fragment_per_workgroup(name, seq):
    ms, base = _base(name, SINGLE[name])
    got = _launch(ms, [seq] * len(ms))
    _check(ms, base, got, "%s seq %d" % (name, seq))
    if name == "straddle-empty-tail":
        assert -(-9 // seq) * seq >= 9 and (seq == 3 or -(-9 // seq) * seq > 9)  # seq 2 and 4 end in an empty tail, every seq straddles crops


@pytest.mark.parametrize("seq", SEQS)
def test_fused_input_runs_match_the_two_launch_form(seq):
    """y and out of the fused-input launch at seq equal i2r_fuse_up_add followed by a plain conv (at seq 1), bit for bit; y prefilled with NaN"""
    ms, _ = _base("fused-input", SINGLE["fused-input"])
    if "fused-two-launch" not in _BASE:
        _BASE["fused-two-launch"] = _launch(ms, [1] * len(ms), fused=False)
    two = _BASE["fused-two-launch"]
    got = _launch(ms, [seq] * len(ms))
    for m, (y0, o0, _), (y1, o1, _) in zip(ms, two, got):
        assert not torch.isnan(y1).any() and torch.equal(y0, y1) and torch.equal(o0, o1), m.tag


@pytest.mark.parametrize("table", [True, False], ids=["table", "banded"])
def test_grouped_stage3_launch_with_a_run_length_per_member(table):
    """48 @ 64x48, 96 @ 32x24, 192 @ 16x12 at 2 crops in one launch, seq 4 / 2 / 1: every workgroup runs 12 passes"""
    make = lambda: [Member(2, 48, 48, 64, 48, "s48", res1=True), Member(2, 96, 96, 32, 24, "s96", res1=True), Member(2, 192, 192, 16, 12, "s192", res1=True)]
    ms, base = _base("stage3", make)
    _check(ms, base, _launch(ms, [4, 2, 1], table=table), "stage3 %s" % ("table" if table else "banded"))


def _resolved(st):
    """run lengths i2r_conv_grid reports for a grouped launch as the engine issues it"""
    arr = (C.POINTER(cabi.ConvDesc) * st.n)(*[st.d[i] for i in range(st.n)])
    g, seqs = C.c_int32(-1), (C.c_int32 * st.n)()
    cabi.check(cabi.lib().i2r_conv_grid(arr, st.n, int(bool(st.block_map)), C.byref(g), seqs), "i2r_conv_grid")
    return list(seqs)


def test_grouped_stage3_launch_at_the_librarys_choice():
    """seq = 0 where the library really strings fragments together: the stage-3 group at 9 crops (540 workgroups with the 48-channel
    fragments in pairs, the fewest crops at which the floor of 512 leaves them paired) against seq 1 and float64"""
    make = lambda: [Member(9, 48, 48, 64, 48, "c48", res1=True), Member(9, 96, 96, 32, 24, "c96", res1=True), Member(9, 192, 192, 16, 12, "c192", res1=True)]
    ms, base = _base("stage3-9", make)
    dev = torch.device(DEV)
    P = engine.Program(dev)
    grp = []
    for m in ms:
        m.emit(P, grp)
    assert all(g[0].seq == 0 for g in grp) and engine.WINO_SEQ
    P.flush_group(grp)
    (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
    assert sorted(zip([st.d[i].contents.cin for i in range(st.n)], _resolved(st))) == [(48, 2), (96, 1), (192, 1)]
    run(P)
    got = [(None, m.out.view().clone(), from_act(m.out).double()) for m in ms]
    _check(ms, base, got, "stage3 at 9 crops, seq 0")


def _model(seq_on, lengths):
    """lengths None: the smallest w48 golden case (1 crop); else synthetic inputs for those persons per image"""
    from i2r_amd import caller
    saved = engine.WINO_SEQ
    engine.WINO_SEQ = seq_on
    try:
        cfg, sd, x, m, length, _ = setup("w48_l1")
        if lengths is not None:
            x, m, length = synth.make_inputs(lengths, 256, 192, seed=5)
        net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
        y = net(x.cuda(), m.cuda(), length).cpu()
        f = net.forward_flip(x.cuda(), m.cuda(), length, caller.FLIP_PAIRS["crowdpose"]).cpu()
        groups = [st for P, *_ in net.engine().programs.values() for k, _, st in P.ops if k == cabi.OP_CONV_GROUP and st.d[0].contents.algo == 1]
        seqs = {st.d[i].contents.seq for st in groups for i in range(st.n)}
        longest = max(max(_resolved(st)) for st in groups)
        return y, f, seqs, longest
    finally:
        engine.WINO_SEQ = saved


@pytest.mark.parametrize("lengths", [None, [4] * 6], ids=["golden-1-crop", "24-crops"])
def test_model_heat_maps_are_bitwise_equal_with_and_without_runs(lengths):
    """plain and flip-test forward, engine.WINO_SEQ on (the library chooses) / off (one fragment): the smallest w48 golden case, where
    every launch is too small for the library to form runs (so both are the same launches), and 24 crops, where it pairs fragments"""
    y0, f0, s0, l0 = _model(False, lengths)
    y1, f1, s1, l1 = _model(True, lengths)
    assert s0 == {1} and s1 == {0} and torch.isfinite(y0).all() and torch.isfinite(f0).all()
    assert l0 == 1 and l1 == (1 if lengths is None else 2), (l0, l1)
    assert torch.equal(y0, y1), "forward: max |d| %.3e" % (y0 - y1).abs().max().item()
    assert torch.equal(f0, f1), "forward_flip: max |d| %.3e" % (f0 - f1).abs().max().item()
