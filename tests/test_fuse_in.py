"""CPU: what the HRNet tower programs contain once the closing pass of a fuse layer (i2r_fuse_up_add) rides in the staging of the next
module's first Winograd conv (engine.FUSE_IN, i2r_conv_desc.t1 / t2 / y) and the last module computes only the outputs its caller reads
(HRNetW48.emit(need=...)).  Programs are built on the CPU device; nothing is launched."""
import contextlib
import ctypes as C

import pytest
import torch

import i2r_amd  # noqa: F401
from i2r_amd import arch, cabi, config, engine, synth

import _conv_cases as cc

E_ARG = -1  # I2R_E_ARG of include/i2r_hip.h
N, H, W = 3, 256, 192


@contextlib.contextmanager
def switches(fuse_in):
    saved = engine.FUSE_IN
    engine.FUSE_IN = fuse_in
    try:
        yield
    finally:
        engine.FUSE_IN = saved


_TOWERS = {}


def tower_of(prec):
    if prec not in _TOWERS:
        cfg = config.load_config("w48_pure_en6")
        sd = synth.make_state_dict(arch.param_spec(cfg))
        pk = engine.Packer(sd, torch.device("cpu"), prec)
        _TOWERS[prec] = (pk, engine.HRNetW48(pk, "", cfg["MODEL"]["EXTRA"]))
    return _TOWERS[prec]


def tower_program(prec, fuse_in, need, **kw):
    pk, tower = tower_of(prec)
    with switches(fuse_in):
        P = engine.Program(torch.device("cpu"))
        P.store_dt = pk.dtype
        xs, _ = tower.emit(P, N, H, W, **({"need": need} if need != "default" else {}), **kw)
    return P, xs


def members(P):
    """per launch: (kind, list of descriptors) of the conv launches, (kind, None) of everything else"""
    out = []
    for kind, _, st in P.ops:
        if kind == cabi.OP_CONV:
            out.append((kind, [st]))
        elif kind == cabi.OP_CONV_GROUP:
            out.append((kind, [st.d[i].contents for i in range(st.n)]))
        else:
            out.append((kind, None))
    return out


def geometry(d):
    return (d.algo, d.n_img, d.in_h, d.in_w, d.cin, d.conv_h, d.conv_w, d.cout, d.stride, d.ntaps, d.relu, d.rep, d.tile_h, d.tile_w, d.mt, d.wn,
            bool(d.res1), bool(d.res2), d.dtype, d.in_f16, d.out_f16)


def igemm_launches(P):
    """the implicit-GEMM launches of a program, in order: (resolved name, geometry of every member)"""
    out = []
    for kind, ds in members(P):
        if ds is None or ds[0].algo == 1:
            continue
        rc, name, err = cc.resolve(ds)
        assert rc == 0, err
        out.append((name, tuple(geometry(d) for d in ds)))
    return out


def n_fuse_up(P):
    return sum(1 for kind, _, _ in P.ops if kind == cabi.OP_FUSE_UP)


def test_fp32_bare_tower_has_no_closing_pass_and_nine_launches_fewer():
    before, _ = tower_program("fp32", False, None)
    after, xs = tower_program("fp32", True, {-1})
    assert n_fuse_up(before) == 9 and n_fuse_up(after) == 0
    assert len(before.ops) - len(after.ops) == 9
    assert xs[0] is None and xs[1] is None and (xs[2].h, xs[2].w, xs[2].c) == (H // 16, W // 16, 192)
    fused = [d for _, ds in members(after) if ds for d in ds if d.t1]
    assert len(fused) == 7  # stage 2's output 0 and outputs 0, 1 of the first three stage-3 modules
    for d in fused:
        assert d.algo == 1 and d.y and d.y not in (d.in_, d.t1, d.t2, d.out) and d.in_cs == d.cin and d.relu == 1
        assert (d.t1_shift, d.t2_shift if d.t2 else 0) in ((1, 0), (1, 2))
    for _, ds in members(after):  # every fused launch resolves, to the fused form of the kernel; the plain ones to the plain form
        if ds and ds[0].algo == 1:
            rc, name, err = cc.resolve(ds)
            assert rc == 0, err
            assert name == ("conv_wino_fin_f32<1, 3>" if any(d.t1 for d in ds) else "conv_wino_f32<1, %d>" % (3 if ds[0].cout_pad % 48 == 0 else 4))


def test_folding_alone_leaves_the_implicit_gemm_launches_unchanged():
    before, _ = tower_program("fp32", False, None)
    folded, xs = tower_program("fp32", True, None)
    assert igemm_launches(folded) == igemm_launches(before)
    assert n_fuse_up(folded) == 2 and all(x is not None for x in xs)  # the two outputs that leave the tower keep their pass
    # the Winograd launches are the same ones too, apart from the fused terms
    wino = lambda P: [tuple(geometry(d) for d in ds) for _, ds in members(P) if ds and ds[0].algo == 1]
    assert wino(folded) == wino(before)


def test_pruning_changes_the_implicit_gemm_launches_only_in_the_last_module():
    for prec, fuse_in in (("fp32", True), ("fp32", False), ("bf16", True)):
        full, _ = tower_program(prec, fuse_in, None)
        pruned, _ = tower_program(prec, fuse_in, {-1})
        a, b = igemm_launches(full), igemm_launches(pruned)
        # the last module's fuse layers are the last two implicit-GEMM launches of the tower (two levels for three branches)
        assert len(a) == len(b) and a[:-2] == b[:-2] and a[-2:] != b[-2:]
        # what is left of them: the two chains into the lowest branch -- fuse(2, 0) (two stride-2 convs) and fuse(2, 1)
        assert [len(g) for _, g in b[-2:]] == [2, 1] and [len(g) for _, g in a[-2:]] == [3, 4]
        assert all(g[8] == 2 and g[9] == 9 for _, gs in b[-2:] for g in gs)
        assert n_fuse_up(full) - n_fuse_up(pruned) == 2
        # an output in the middle: its own terms stay, the others go
        mid, xs = tower_program(prec, fuse_in, {1})
        assert xs[0] is None and xs[2] is None and xs[1].c == 96
        # the block convs of every branch stay: the needed output depends on all of them
        blocks = lambda P: sum(len(ds) for _, ds in members(P) if ds and all(d.ntaps == 9 and d.stride == 1 for d in ds))
        assert blocks(full) == blocks(pruned) == blocks(mid)


def test_bf16_tower_keeps_its_closing_passes():
    off, _ = tower_program("bf16", False, None)
    on, _ = tower_program("bf16", True, None)
    assert n_fuse_up(on) == n_fuse_up(off) == 9
    assert [k for k, _, _ in on.ops] == [k for k, _, _ in off.ops]
    assert not any(d.t1 or d.t2 or d.y for _, ds in members(on) if ds for d in ds)
    pruned, _ = tower_program("bf16", True, {-1})
    assert n_fuse_up(pruned) == 7


def test_emit_with_default_arguments_gives_the_unpruned_tower():
    """emit(P, n, h, w) as tests/test_conv_dispatch.py calls it: every output, the launches of need=None"""
    for prec in ("fp32", "bf16"):
        dflt, xs = tower_program(prec, True, "default")
        full, _ = tower_program(prec, True, None)
        assert all(x is not None for x in xs)
        assert [k for k, _, _ in dflt.ops] == [k for k, _, _ in full.ops]
        assert igemm_launches(dflt) == igemm_launches(full)
        off, _ = tower_program(prec, False, "default")
        assert igemm_launches(off) == igemm_launches(dflt)


def test_prune_switch_keeps_every_output():
    """the switch PRUNE_FUSE turns the pruning off whatever the caller asks for (tests build both forms of a model with it)"""
    pk, tower = tower_of("fp32")
    saved = engine.PRUNE_FUSE
    try:
        engine.PRUNE_FUSE = False
        P = engine.Program(torch.device("cpu"))
        xs, _ = tower.emit(P, N, H, W, need={-1})
        assert all(x is not None for x in xs)
    finally:
        engine.PRUNE_FUSE = saved


def _fused_descs():
    P, _ = tower_program("fp32", True, {-1})
    return [ds for _, ds in members(P) if ds and any(d.t1 for d in ds)]


def _copy(d):
    c = cabi.ConvDesc()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(cabi.ConvDesc))
    return c


@pytest.mark.parametrize("field", ["in_", "t1", "t2", "out"])
def test_y_aliasing_another_tensor_is_refused(field):
    ds = next(g for g in _fused_descs() if any(d.t2 for d in g))
    i = next(i for i, d in enumerate(ds) if d.t2)
    bad = [_copy(d) for d in ds]
    bad[i].y = getattr(bad[i], field)
    rc, _, err = cc.resolve(bad)
    assert rc == E_ARG and "aliases" in err, err
    assert cc.resolve([_copy(d) for d in ds])[0] == 0


def test_fused_input_argument_errors():
    ds = next(g for g in _fused_descs() if any(d.t2 for d in g))
    i = next(i for i, d in enumerate(ds) if d.t2)

    def refused(**kw):
        bad = [_copy(d) for d in ds]
        for k, v in kw.items():
            setattr(bad[i], k, v)
        rc, _, err = cc.resolve([bad[i]])
        return rc == E_ARG, err
    assert refused(y=None)[0]                       # terms without a destination
    assert refused(t1=None)[0]                      # t2 / y without t1
    assert refused(t1_shift=3)[0] and refused(t2_shift=0)[0]
    assert refused(in_h=ds[i].in_h + 2, conv_h=ds[i].conv_h + 2, out_h=ds[i].out_h + 2)[0]  # map not divisible by 4
    assert refused(in_cs=ds[i].in_cs + 16)[0]       # channels the conv does not read would be missing from y
    assert refused(algo=0, tile_h=0, tile_w=0, mt=0)[0]  # Winograd only
    # 16-bit storage is refused by the Winograd kernels as before
    lp = cc.CASES[next(j for j, c in enumerate(cc.CASES) if c.dtype == 1)].desc()
    lp.t1, lp.y, lp.t1_shift = 0x90000, 0xA0000, 1
    rc, _, err = cc.resolve([lp])
    assert rc == E_ARG, err


def test_program_conv_refuses_fuse_in_where_the_kernel_cannot_fold():
    P = engine.Program(torch.device("cpu"))
    pk, tower = tower_of("bf16")
    pc = tower.stage3[0]["blocks"][0][0][0]
    x, t, y = P.alloc(2, 64, 48, 48, 1), P.alloc(2, 32, 24, 48, 1), P.alloc(2, 64, 48, 48, 1)
    assert not P.fuse_in_ok(x, [t], pc)
    with pytest.raises(ValueError):
        P.conv(x, pc, relu=True, fuse_in=([t], y))
    pk32, tower32 = tower_of("fp32")
    pc = tower32.stage3[0]["blocks"][0][0][0]
    x, t8, y = P.alloc(2, 64, 48, 48), P.alloc(2, 8, 6, 48), P.alloc(2, 64, 48, 48)
    assert not P.fuse_in_ok(x, [t8], pc)  # a term at 1/8 of the map
    assert P.fuse_in_ok(x, [P.alloc(2, 32, 24, 48), P.alloc(2, 16, 12, 48)], pc)
