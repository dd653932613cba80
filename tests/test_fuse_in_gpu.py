"""-m gpu: the closing pass of an HRNet fuse layer folded into the staging of a Winograd conv (i2r_conv_desc.t1 / t2 / y,
csrc/i2r_conv_wino.hip) against the two launches it replaces -- bitwise -- and against float64; the pruned last module of the tower."""
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
E_ARG = -1  # I2R_E_ARG of include/i2r_hip.h


def _rand(shape, key, scale=1.0):
    return torch.from_numpy(synth._sym(11, key, tuple(shape), scale))


def _conv_sd(cin, cout, tag):
    return {"c.weight": _rand((cout, cin, 3, 3), "w" + tag, (6.0 / (cin * 9)) ** 0.5),
            "b.weight": _rand((cout,), "g" + tag, 0.5) + 1.0, "b.bias": _rand((cout,), "b" + tag, 0.3),
            "b.running_mean": _rand((cout,), "m" + tag, 0.3), "b.running_var": _rand((cout,), "v" + tag, 0.4) + 1.0}


class Member:
    """one conv of a launch: base map, up-sampled terms (scales; () = a plain member), weights, float64 references"""

    def __init__(self, n, cin, cout, h, w, scales, tag):
        self.scales, self.tag = scales, tag
        self.sd = _conv_sd(cin, cout, tag)
        self.base = _rand((n, cin, h, w), "x" + tag)
        self.terms = [_rand((n, cin, h // s, w // s), "t%d%s" % (s, tag)) for s in scales]
        y = self.base.double()
        for t, s in zip(self.terms, scales):
            y = y + F.interpolate(t.double(), scale_factor=s, mode="nearest")
        self.y_ref = F.relu(y) if scales else y
        sd = {k: v.double() for k, v in self.sd.items()}
        ref = F.conv2d(self.y_ref, sd["c.weight"], None, padding=1)
        self.ref = F.relu(F.batch_norm(ref, sd["b.running_mean"], sd["b.running_var"], sd["b.weight"], sd["b.bias"], False, 0.0, 1e-5))

    def emit(self, P, fused, grp):
        pc = engine.Packer(self.sd, torch.device(DEV)).conv("c", "b")
        self.acts = [to_act(P, self.base)] + [to_act(P, t) for t in self.terms]
        base, terms = self.acts[0], self.acts[1:]
        if not self.scales:
            self.y = base
            self.out = P.conv(base, pc, relu=True, group=grp)
            return
        self.y = P.alloc(base.n, base.h, base.w, base.c)
        self.y.t.fill_(float("nan"))
        if fused:
            self.out = P.conv(base, pc, relu=True, group=grp, fuse_in=(terms, self.y))
        else:
            P.fuse_up_add(base, terms, self.y, relu=True)
            self.out = P.conv(self.y, pc, relu=True, group=grp)

    def inputs_unchanged(self):
        return all(torch.equal(from_act(a), t) for a, t in zip(self.acts, [self.base] + self.terms))


def _launch(ms, fused):
    P = engine.Program(torch.device(DEV))
    grp = []
    for m in ms:
        m.emit(P, fused, grp)
    P.flush_group(grp)
    groups = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
    assert len(groups) == 1 and groups[0].n == len(ms) and all(groups[0].d[i].contents.algo == 1 for i in range(len(ms)))
    by_out = {groups[0].d[i].contents.out: groups[0].d[i].contents for i in range(len(ms))}  # (flush_group puts the heaviest member first)
    descs = [by_out[m.out.ptr] for m in ms]
    assert sum(1 for d in descs if d.t1) == (sum(1 for m in ms if m.scales) if fused else 0)
    rc, name, err = cc.resolve(descs)
    assert rc == 0 and name == ("conv_wino_fin_f32<1, 3>" if fused else "conv_wino_f32<1, 3>"), (name, err)
    assert sum(1 for k, _, _ in P.ops if k == cabi.OP_FUSE_UP) == (0 if fused else sum(1 for m in ms if m.scales))
    run(P)
    res = [(m.y.view().clone(), m.out.view().clone(), from_act(m.out).double(), m.inputs_unchanged()) for m in ms]
    return res, descs


def _check(ms, frag_w=None):
    plain, _ = _launch(ms, False)
    fused, descs = _launch(ms, True)
    if frag_w is not None:
        assert [d.tile_w for d in descs] == frag_w  # fragment shapes: 16, 8 or 4 pixels wide
    for m, (y0, o0, _, _), (y1, o1, got, same) in zip(ms, plain, fused):
        assert same, "%s: the fused launch changed base / t1 / t2" % m.tag
        assert not torch.isnan(y1).any() and not torch.isnan(o1).any(), "%s: y not written completely" % m.tag
        assert torch.equal(y0, y1), "%s: y differs from i2r_fuse_up_add, max |d| %.3e" % (m.tag, (y0 - y1).abs().max().item())
        assert torch.equal(o0, o1), "%s: conv output differs from fuse_up_add + conv, max |d| %.3e" % (m.tag, (o0 - o1).abs().max().item())
        if m.scales:
            assert (from_act(m.y).double() - m.y_ref).abs().max().item() < 1e-6 * max(1.0, m.y_ref.abs().max().item())
        err = (got - m.ref).abs().max().item()
        bar = 2e-5 * max(1.0, m.ref.abs().max().item())  # the bar of test_conv_winograd_matches_torch_and_direct
        print("%s: conv max |got - ref| %.3e (bar %.3e)" % (m.tag, err, bar))
        assert err < bar, "%s: max-abs %.3e" % (m.tag, err)


@pytest.mark.parametrize("h,w,scales,cout,frag_w", [
    (16, 12, (2, 4), 48, 4),    # FW = 2: 4 x 16-pixel fragments, terms 8x6 and 4x3
    (32, 24, (2,), 48, 8),      # FW = 4, one term at 16x12
    (64, 48, (2, 4), 48, 16),   # FW = 8, two terms
    (32, 24, (2, 4), 96, 8),    # two channel blocks: only block 0 stores y
], ids=["16x12-fw2", "32x24-fw4", "64x48-fw8", "cout96"])
def test_fused_input_matches_fuse_up_add_then_conv_bitwise(h, w, scales, cout, frag_w):
    """3 crops, cin = 48 (three 16-channel passes); y prefilled with NaN"""
    _check([Member(3, 48, cout, h, w, scales, "fi%d_%d_%d_%d" % (h, w, cout, len(scales)))], [frag_w])


def test_grouped_launch_of_fused_and_plain_members():
    """block 1 of a stage-3 module: branches 0 and 1 fold their closing passes, the lowest branch has none"""
    _check([Member(3, 48, 48, 64, 48, (2, 4), "g0"), Member(3, 96, 96, 32, 24, (2,), "g1"), Member(3, 192, 192, 16, 12, (), "g2")], [16, 8, 4])


def test_y_aliasing_base_is_refused_before_any_launch():
    m = Member(2, 48, 48, 16, 12, (2,), "alias")
    P = engine.Program(torch.device(DEV))
    grp = []
    m.emit(P, True, grp)
    d = grp[0][0]
    out = m.out.view()
    out.fill_(5.0)
    d.y = d.in_
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    assert cabi.lib().i2r_conv(C.byref(d), stream) == E_ARG
    assert b"aliases" in cabi.lib().i2r_last_error()
    torch.cuda.synchronize()
    assert (out == 5.0).all() and torch.equal(from_act(m.acts[0]), m.base)


# ------------------------------------------------------------------------------------------------------------------------------
# the model: folded / unfolded, pruned / unpruned
# ------------------------------------------------------------------------------------------------------------------------------
def _model_outputs(fuse_in, prune):
    from i2r_amd import caller
    saved = engine.FUSE_IN, engine.PRUNE_FUSE
    engine.FUSE_IN, engine.PRUNE_FUSE = fuse_in, prune
    try:
        cfg, sd, _, _, _, _ = setup("w48_l1")
        net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
        x, m, length = synth.make_inputs([2, 1], 256, 192, seed=3)
        y = net(x.cuda(), m.cuda(), length).cpu()
        f = net.forward_flip(x.cuda(), m.cuda(), length, caller.FLIP_PAIRS["crowdpose"]).cpu()
        progs = [P for P, *_ in net.engine().programs.values()]
        n_close = sum(1 for P in progs for k, _, _ in P.ops if k == cabi.OP_FUSE_UP)
        n_fused = sum(1 for P in progs for k, _, st in P.ops if k == cabi.OP_CONV_GROUP for i in range(st.n) if st.d[i].contents.t1)
        n_towers = sum(1 for P in progs if any(k == cabi.OP_STEM for k, _, _ in P.ops))
        return y, f, n_close, n_fused, n_towers
    finally:
        engine.FUSE_IN, engine.PRUNE_FUSE = saved


def test_model_heat_maps_are_bitwise_equal_folded_and_pruned():
    """w48_pure_en6, 3 crops (lengths [2, 1]) at 256x192, plain and flip-test forward: FUSE_IN on / off x pruned / unpruned"""
    ref = _model_outputs(False, False)
    assert ref[0].shape == (3, 14, 64, 48) and torch.isfinite(ref[0]).all() and ref[3] == 0 and ref[4] >= 2 and ref[2] == 9 * ref[4]
    for fuse_in, prune in ((True, True), (True, False), (False, True)):
        got = _model_outputs(fuse_in, prune)
        assert torch.equal(got[0], ref[0]), "forward, FUSE_IN %r pruned %r: max |d| %.3e" % (fuse_in, prune, (got[0] - ref[0]).abs().max().item())
        assert torch.equal(got[1], ref[1]), "forward_flip, FUSE_IN %r pruned %r: max |d| %.3e" % (fuse_in, prune, (got[1] - ref[1]).abs().max().item())
        assert got[4] == ref[4]
        assert got[2] == (9 - (7 if fuse_in else 0) - (2 if prune else 0)) * ref[4] and got[3] == (7 * ref[4] if fuse_in else 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the implicit-GEMM launches only the pruned last module emits, through the C-ABI against float64
# ------------------------------------------------------------------------------------------------------------------------------
def _case_of(d, name, tag):
    """a cc.Case with the geometry of an engine-built descriptor (its operands come from cc.make_tensors)"""
    taps = [(d.dy[i], d.dx[i]) for i in range(d.ntaps)]
    return cc.Case(name=name, tag=tag, n=d.n_img, in_h=d.in_h, in_w=d.in_w, in_cs=d.in_cs, cin=d.cin, conv_h=d.conv_h, conv_w=d.conv_w,
                   out_h=d.out_h, out_w=d.out_w, out_cs=d.out_cs, cout=d.cout, cout_pad=d.cout_pad, stride=d.stride, iy0=d.iy0, ix0=d.ix0,
                   taps=taps, tile_h=d.tile_h, tile_w=d.tile_w, mt=d.mt, wn=d.wn, ck=d.ck, dtype=d.dtype, in16=d.in_f16, out16=d.out_f16,
                   relu=d.relu, out_step=d.out_step, out_off=(d.out_off_y, d.out_off_x), rep=d.rep, in2=bool(d.in2),
                   nres=int(bool(d.res1)) + int(bool(d.res2)), inplace=bool(d.res1) and d.res1 == d.out, res_post=bool(d.res_post))


def _pruned_only_launches():
    """[(id, resolved name, member descriptors, dispatch table or None)]: built on the CPU device, nothing launched"""
    from i2r_amd import arch, config
    out = []
    for prec in ("fp32", "bf16"):
        cfg = config.load_config("w48_pure_en6")
        sd = synth.make_state_dict(arch.param_spec(cfg))
        pk = engine.Packer(sd, torch.device("cpu"), prec)
        tower = engine.HRNetW48(pk, "", cfg["MODEL"]["EXTRA"])
        for need in ({-1}, {0}):  # the bare tower's lowest branch; TransPose-H's HRNET_RES_LAYER 0
            launches = {}
            for which in (None, need):
                P = engine.Program(torch.device("cpu"))
                P.store_dt = pk.dtype
                tower.emit(P, 3, 256, 192, need=which)
                ls = []
                for kind, _, st in P.ops:
                    if kind == cabi.OP_CONV:
                        ds, bm = [st], None
                    elif kind == cabi.OP_CONV_GROUP:
                        ds, bm = [st.d[i].contents for i in range(st.n)], (st.block_map, st.map_len)
                    else:
                        continue
                    if ds[0].algo == 0:
                        sig = tuple((d.in_h, d.in_w, d.cin, d.cout, d.stride, d.ntaps, d.relu, d.tile_h, d.tile_w, d.mt, d.wn, bool(d.res1),
                                     bool(d.res1) and d.res1 == d.out) for d in ds)
                        ls.append((sig, ds, bm, P))
                launches[which is None] = ls
            seen = {sig for sig, _, _, _ in launches[True]}
            for sig, ds, bm, P in launches[False]:
                if sig not in seen:
                    seen.add(sig)
                    rc, name, err = cc.resolve(ds)
                    assert rc == 0, err
                    table = None
                    if bm[0] if bm else False:
                        t = next(k for k in P.keep if torch.is_tensor(k) and k.dtype == torch.int32 and k.data_ptr() == bm[0])
                        table = t.tolist()
                    out.append(("%s-need%d-%dx" % (prec, sorted(need)[0], len(ds)) + "+".join("%d>%d" % (d.cin, d.cout) for d in ds), name, ds, table, P))
    return out


_PRUNED = _pruned_only_launches()


def test_pruning_emits_launches_of_its_own():
    assert len(_PRUNED) >= 4 and len({p[0] for p in _PRUNED}) == len(_PRUNED)


@pytest.mark.parametrize("launch", _PRUNED, ids=[p[0] for p in _PRUNED])
def test_pruned_module_launches_match_float64(launch):
    """as tests/test_kernels_gpu.py::test_conv_every_instantiation_matches_float64 / ..._grouped_...: the descriptor geometry the engine built,
    operands and guarded outputs of tests/_conv_cases.py, its float64 reference and its bars"""
    lid, name, ds, table, _ = launch
    dev = torch.device(DEV)
    cases = [_case_of(d, name, "%s-m%d" % (lid, j)) for j, d in enumerate(ds)]
    ts = [cc.make_tensors(c) for c in cases]
    args = [cc.launch_args(c, t, dev) for c, t in zip(cases, ts)]
    descs = [a[0] for a in args]
    rc, got_name, err = cc.resolve(descs)
    assert rc == 0 and got_name == name, (got_name, err)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if len(descs) == 1 and table is None:
        cabi.check(cabi.lib().i2r_conv(C.byref(descs[0]), stream), "i2r_conv")
    else:
        bmd = torch.tensor(table, dtype=torch.int32, device=dev) if table is not None else None
        arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
        cabi.check(cabi.lib().i2r_conv_grouped(arr, len(descs), bmd.data_ptr() if bmd is not None else None, len(table) if table else 0, stream),
                   "i2r_conv_grouped")
    torch.cuda.synchronize()
    for c, t, a in zip(cases, ts, args):
        cc.check_output(c, t, a[1].cpu())
