"""CPU: which conv instantiation a descriptor resolves to (i2r_conv_kernel_name launches nothing), for the case table of _conv_cases.py,
for everything the engine's cost model proposes, and for the argument errors of prepare() / resolve() (csrc/i2r_conv_plan.h)."""
import collections
import ctypes as C
import re

import pytest
import torch

import i2r_amd  # noqa: F401
from i2r_amd import arch, cabi, config, engine, synth

import _conv_cases as cc

E_ARG = -1  # I2R_E_ARG of include/i2r_hip.h
CROPS = (3, 6, 12, 16, 32, 57, 64)  # the golden size, the bench.WORKLOADS sizes (16, 32, 12 -> capacity 16) and their flip-test doubles
SIZES = ((256, 192), (384, 288))
FAMILY = cc.CASES[:len(cc.all_names())]  # the table proper: one case per instantiation (the rest pair an instantiation with the engine's wn)


# ------------------------------------------------------------------------------------------------------------------------------
# the table means what it says
# ------------------------------------------------------------------------------------------------------------------------------
def test_every_case_resolves_to_the_instantiation_it_names():
    expected = cc.all_names()
    assert len(expected) == 144
    for c in cc.CASES:
        rc, name, err = cc.resolve([c.desc()])
        assert rc == 0, "%s rejected: %s" % (c.id, err)
        assert name == c.name, "%s resolves to %s" % (c.id, name)
    assert {c.name for c in FAMILY} == expected and len(FAMILY) == 144
    assert len({c.id for c in cc.CASES}) == len(cc.CASES)


def test_every_group_resolves_to_its_common_variant():
    for g in cc.GROUP_CASES:
        descs = [m.desc(out=0x40000 + 0x100000 * j) for j, m in enumerate(g.members)]
        rc, name, err = cc.resolve(descs)
        assert rc == 0, "%s rejected: %s" % (g.id, err)
        assert name == g.name, "%s resolves to %s" % (g.id, name)
        for m, d in zip(g.members, descs):
            assert cc.resolve([d])[1] == m.name  # what the member would run alone
        bm = g.block_map()
        if bm is not None:  # a permutation of every (member, workgroup)
            assert sorted(bm) == [(gi << 24) | i for gi, n in enumerate(g.counts()) for i in range(n)]
    assert len({g.id for g in cc.GROUP_CASES}) == len(cc.GROUP_CASES)


def test_cases_stress_the_instantiations():
    """the properties the table promises, so that an edit of the generator cannot quietly drop one"""
    for c in cc.CASES:
        assert c.n >= 2 and c.conv_h % c.tile_h and c.conv_w % c.tile_w, c.id  # partial tiles in both directions
        assert c.cout < c.cout_pad and c.tile_h * c.tile_w <= (4 // c.wn) * c.mt * 16, c.id
        assert c.n * c.out_h * c.out_w <= 16384, c.id  # (tiny launches)
        if c.variant[1] >= 1:
            assert c.chunks >= 3, c.id
    for dt in (0, 1, 2):
        fam = [c for c in FAMILY if c.dtype == dt]
        for mt in cc.MTS:
            px = [c.tile_h * c.tile_w for c in fam if c.mt == mt]
            assert any(p % 16 for p in px), "MT %d: no partly filled last fragment" % mt
            assert any(c.full for c in fam if c.mt == mt), "MT %d: no case that fills every fragment" % mt
        for nt in cc.NTS:
            assert any(c.n_cblk > 1 for c in fam if cc.kernel_name(dt, c.mt, nt, *c.variant) == c.name), "NT %d: one channel block only" % nt
        for cap, pf in cc.variants(dt):
            par = {c.chunks % 2 for c in fam if c.variant == (cap, pf)}
            assert pf == 0 or par == {0, 1}, "dtype %d (%d, %d): chunk counts of one parity only" % (dt, cap, pf)
        for c in fam:
            if c.variant[1] == 2:
                assert c.stride == 2 and c.in_h % 2 == 1 and c.in_w % 2 == 1, c.id
        if dt == 0:
            assert any(c.ck and c.cin % c.ck for c in fam if c.variant[1] == 0), "PF 0: no short last chunk"
            assert any(c.patch > 1024 for c in fam if c.variant[1] == 0), "PF 0: no patch of five pixels per thread"
        feats = set(cc.FEATURES if dt == 0 else cc.lp_features())
        assert feats <= {c.feature for c in fam if c.mt >= 2}, "dtype %d: %s never meet MT >= 2" % (dt, feats - {c.feature for c in fam if c.mt >= 2})
        everyone = [c for c in cc.CASES if c.dtype == dt] + [m for g in cc.GROUP_CASES for m in g.members if m.dtype == dt]
        assert {(0, 0), (0, 1), (1, 0), (1, 1)} == {c.out_off for c in everyone if c.feature == "deconv"}
        if dt:
            assert {(0, 0), (0, 1), (1, 0), (1, 1)} == {(c.in16, c.out16) for c in fam if c.mt >= 2}
    # grouped launches: 2, 3 and 4 members, every dispatch-table mode, and the forced-variant paths of resolve()
    assert {len(g.members) for g in cc.GROUP_CASES} == {2, 3, 4}
    assert {g.map for g in cc.GROUP_CASES} == {None, "lpt", "reversed", "interleaved"}
    forced = collections.Counter()
    for g in cc.GROUP_CASES:
        assert any(m.name == g.name for m in g.members)  # one member needs the common variant; the others are forced onto it
        for m in g.members:
            if m.variant != g.variant:
                forced[(m.variant, g.variant)] += 1
        assert len({m.mt for m in g.members}) == 1 and len({m.dtype for m in g.members}) == 1
    assert {m.mt for g in cc.GROUP_CASES for m in g.members} >= {2, 3}
    for v in ((12, 1), (8, 1), (4, 2), (4, 0)):  # the member that needs the common variant is not always the first
        assert any(g.variant == v and g.members[0].variant != v for g in cc.GROUP_CASES), v
    for dt_wide in (12, 8):
        assert forced[((4, 1), (4, 2))] and forced[((4, 1), (dt_wide, 1))] and forced[((4, 1), (4, 0))], forced
    assert any(len({m.wn for m in g.members}) > 1 and len({m.cin for m in g.members}) > 1 and len({m.stride for m in g.members}) > 1
               and len({len(m.taps) for m in g.members}) > 1 for g in cc.GROUP_CASES)


# ------------------------------------------------------------------------------------------------------------------------------
# the engine only picks what is covered
# ------------------------------------------------------------------------------------------------------------------------------
def program_signatures(P):
    """(resolved name, wn per member, member count, dispatch table?) of every implicit-GEMM launch of a program (the Winograd launches,
    algo 1, are another family: tests/test_kernels_gpu.py::test_conv_winograd_matches_torch_and_direct)"""
    out = []
    for kind, _, st in P.ops:
        if kind == cabi.OP_CONV:
            ds, has_map = [st], False
        elif kind == cabi.OP_CONV_GROUP:
            ds, has_map = [st.d[i].contents for i in range(st.n)], bool(st.block_map)
        else:
            continue
        if ds[0].algo == 1:
            continue
        rc, name, err = cc.resolve(ds)
        assert rc == 0, "the engine built a conv launch the library refuses: %s" % err
        out.append((name, tuple(d.wn for d in ds), len(ds), has_map))
    return out


def engine_inventory():
    """{signature: set of (tower, precision, input height, crops)} over the shipped tower kinds, precisions, input sizes and crop counts,
    plus the conv paths around the towers: reduce, the deconv parity groups, layer1 without the fused 1x1 pairs, the nearest-upsample
    fuse form.  Programs are built on the CPU device; nothing is launched."""
    dev = torch.device("cpu")
    inv = collections.defaultdict(set)
    for prec in ("fp32", "bf16", "fp16"):
        for kind, cname, prefix in (("hrnet", "w48_pure_en6", ""), ("hrformer", "hrt_192_p4_b4", "singleformer.")):
            cfg = config.load_config(cname)
            sd = synth.make_state_dict(arch.param_spec(cfg))
            pk = engine.Packer(sd, dev, prec)
            tower = engine.HRNetW48(pk, prefix, cfg["MODEL"]["EXTRA"]) if kind == "hrnet" else engine.HRFormerB(pk, prefix)
            if kind == "hrnet":
                reduce, dc = pk.conv("reduce"), pk.deconv("deconv_layers.0", "deconv_layers.1")
            for h, w in SIZES:
                for n in CROPS:
                    for pair in ((True, False) if (kind == "hrnet" and prec == "fp32") else (True,)):
                        saved = engine.PAIR1X1
                        engine.PAIR1X1 = pair
                        try:
                            P = engine.Program(dev)
                            P.store_dt = pk.dtype
                            xs, _ = tower.emit(P, n, h, w)
                        finally:
                            engine.PAIR1X1 = saved
                        if kind == "hrnet":
                            fuse = tower.stage3[0]["fuse"]
                            P.conv(xs[1], fuse[(0, 1)], res1=xs[0], up=2)             # the fuse sums as scattering epilogues
                            P.conv(xs[2], fuse[(0, 2)], relu=True, res1=xs[0], up=4)
                            f = P.conv(xs[-1], reduce, out_dt=0)
                            P.deconv(P.deconv(f, dc), dc)
                        for s in program_signatures(P):
                            inv[s].add((kind, prec, h, n))
    return inv


def covered_signatures():
    return {(c.name, (c.wn,), 1, False) for c in cc.CASES} | {g.signature for g in cc.GROUP_CASES}


def test_engine_only_launches_what_the_cases_cover():
    inv = engine_inventory()
    have = covered_signatures()
    missing = sorted(s for s in inv if s not in have)
    assert not missing, "the engine launches %d conv signature(s) no case of tests/_conv_cases.py runs against the reference:\n%s" % (
        len(missing), "\n".join("  %r  e.g. %r" % (s, sorted(inv[s])[0]) for s in missing))
    assert len(inv) > 50  # (the inventory is not vacuous)


def inventory_table():
    """markdown rows for DESIGN.md: per precision, the instantiations the shipped towers select and at which crop counts"""
    inv = engine_inventory()
    per = collections.defaultdict(lambda: collections.defaultdict(set))
    for (name, wns, n, has_map), where in inv.items():
        for kind, prec, h, crops in where:
            per[prec][name].add(crops)
    lines = []
    for prec in ("fp32", "bf16", "fp16"):
        for name in sorted(per[prec]):
            lines.append("| %s | `%s` | %s |" % (prec, name, ", ".join(str(c) for c in sorted(per[prec][name]))))
    used = {name for prec in per for name in per[prec]}
    return lines, sorted(cc.all_names() - used)


# ------------------------------------------------------------------------------------------------------------------------------
# the cost model never proposes what the library refuses
# ------------------------------------------------------------------------------------------------------------------------------
def _sizes():
    s = set(range(1, 21))
    for m in (24, 32, 36, 48, 64):
        s |= {m - 1, m, m + 1}
    return sorted(s | {70})


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [1, 3])
def test_choose_tile_is_accepted_by_the_library(stride, k):
    taps = [(dy, dx) for dy in range(k) for dx in range(k)]
    n_checked = 0
    for wm in (1, 2, 4):
        wn = 4 // wm
        cout_pad = 48 * wn  # NT 3, one channel block
        for conv_h in _sizes():
            for conv_w in _sizes():
                in_h, in_w = (conv_h, conv_w) if stride == 1 else (2 * conv_h - 1, 2 * conv_w - 1)
                for n_img in (1, 3, 16, 64):
                    for force_mt in (0, 1, 2, 3, 4):
                        try:
                            th, tw, mt = engine.choose_tile(conv_h, conv_w, wm, stride, k - 1, n_img, 1, force_mt=force_mt)
                        except AssertionError:
                            assert force_mt, "no tile at all for %dx%d" % (conv_h, conv_w)
                            continue
                        assert th * tw <= wm * mt * 16 and (not force_mt or mt == force_mt)
                        d = cc.make_desc(n_img=n_img, in_h=in_h, in_w=in_w, in_cs=16, cin=16, conv_h=conv_h, conv_w=conv_w, out_h=conv_h,
                                         out_w=conv_w, out_cs=cout_pad, cout=cout_pad, cout_pad=cout_pad, stride=stride, iy0=-(k // 2),
                                         ix0=-(k // 2), taps=taps, tile_h=th, tile_w=tw, mt=mt, wn=wn)
                        rc, name, err = cc.resolve([d])
                        assert rc == 0, "choose_tile(%d, %d, wm %d, stride %d, k %d, n %d, force_mt %d) = (%d, %d, %d): %s" % (
                            conv_h, conv_w, wm, stride, k, n_img, force_mt, th, tw, mt, err)
                        assert name.startswith("conv_igemm_f32<%d, 3," % mt)
                        n_checked += 1
    assert n_checked > 10000


def test_conv_split_agrees_with_the_library():
    for cout_pad in range(48, 1249, 16):
        try:
            nt, wn = engine.conv_split(cout_pad)
        except StopIteration:
            nt = wn = None
        args = dict(n_img=1, in_h=8, in_w=8, in_cs=16, cin=16, conv_h=8, conv_w=8, out_h=8, out_w=8, out_cs=cout_pad, cout=cout_pad,
                    cout_pad=cout_pad, stride=1, iy0=0, ix0=0, taps=[(0, 0)])
        rc, name, err = cc.resolve([cc.make_desc(**args)])
        assert (rc == 0) == (nt is not None), "cout_pad %d: engine %r, library rc %d %s" % (cout_pad, nt, rc, err)
        if rc == 0:
            assert int(re.match(r"conv_igemm_f32<\d, (\d),", name).group(1)) == nt, (cout_pad, name, nt)
            rc, name, err = cc.resolve([cc.make_desc(wn=wn, **args)])
            assert rc == 0 and int(re.match(r"conv_igemm_f32<\d, (\d),", name).group(1)) == nt, (cout_pad, wn, err)
        else:
            assert "multiple of 48, 64 or 80" in err


# ------------------------------------------------------------------------------------------------------------------------------
# argument errors
# ------------------------------------------------------------------------------------------------------------------------------
def _ok_args(**over):
    a = dict(n_img=2, in_h=12, in_w=12, in_cs=32, cin=32, conv_h=12, conv_w=12, out_h=12, out_w=12, out_cs=48, cout=48, cout_pad=48, stride=1,
             iy0=-1, ix0=-1, taps=[(dy, dx) for dy in range(3) for dx in range(3)], tile_h=8, tile_w=8, mt=1, wn=1)
    a.update(over)
    return a


def test_the_base_descriptor_of_the_error_cases_is_accepted():
    assert cc.resolve([cc.make_desc(**_ok_args())]) == (0, "conv_igemm_f32<1, 3, 12, 1>", "")


@pytest.mark.parametrize("over,msg", [
    (dict(tile_h=9, tile_w=8), "does not fit"),                                  # 72 pixels in a 4 x 1 x 16 workgroup
    (dict(wn=2), "does not divide"),                                             # 3 fragments / NT 3 = 1 block for 2 waves
    (dict(taps=[(0, 0), (0, 2)]), "dense"),                                      # a hole in the tap grid
    (dict(tile_h=2, tile_w=128, mt=4, stride=2, in_h=23, in_w=23), "too large"),  # patch 5 x 257 > 1280 pixels
    (dict(out=0x10000), "aliases"),                                              # out == in
    (dict(in2=0x40000), "aliases"),                                              # out == in2
    (dict(in_f16=1), "16-bit activation storage"),
    (dict(out_f16=1), "16-bit activation storage"),
    (dict(dtype=1, in2=0x50000), "dtype"),
    (dict(cin=24), "multiple of 16"),
    (dict(cout_pad=112, cout=112, out_cs=112), "multiple of 48, 64 or 80"),
    (dict(ck=24), "ck="),
    (dict(out_step=2), "destination grid"),
    (dict(in_=None), "null pointer"),
    (dict(stride=3), "stride 3"),
    (dict(taps=[]), "ntaps 0"),
    (dict(rep=0), "rep/out_step"),
    (dict(taps=[(-1, 0)]), "negative tap offset"),
    (dict(algo=2), "algo 2"),
    (dict(dtype=2, in_f16=1, in_cs=36), "in_cs % 8"),
    (dict(dtype=3), "dtype 3"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_prepare_rejects(over, msg):
    rc, name, err = cc.resolve([cc.make_desc(**_ok_args(**over))])
    assert rc == E_ARG and name is None and msg in err, (rc, err)


@pytest.mark.parametrize("second,msg", [
    (dict(dtype=1), "mix compute dtypes"),
    (dict(algo=1), "mix algorithms"),
    (dict(cout=64, cout_pad=64, out_cs=64), "fragment blocking"),   # NT 4 beside NT 3
    (dict(tile_h=16, tile_w=8, mt=2), "does not fit"),              # the group runs on the first member's mt
], ids=lambda v: v if isinstance(v, str) else "")
def test_grouped_members_must_agree(second, msg):
    descs = [cc.make_desc(**_ok_args()), cc.make_desc(**_ok_args(out=0x90000, **second))]
    rc, name, err = cc.resolve(descs)
    assert rc == E_ARG and msg in err, (rc, err)


def test_grouped_rejects_a_wrong_map_len_before_any_launch():
    """i2r_conv_grouped itself, with arguments it refuses before it touches the device: 2 x (2 x 2 tiles x 2 images) = 16 workgroups"""
    L = cabi.lib()
    descs = [cc.make_desc(**_ok_args()), cc.make_desc(**_ok_args(out=0x90000))]
    arr = (C.POINTER(cabi.ConvDesc) * 2)(*[C.pointer(d) for d in descs])
    for map_len in (15, 17, 0):
        assert L.i2r_conv_grouped(arr, 2, 0xA0000, map_len, None) == E_ARG
        assert b"block_map has %d entries, grid has 16" % map_len in L.i2r_last_error()
    assert L.i2r_conv_grouped(arr, 5, None, 0, None) == E_ARG and b"descriptors" in L.i2r_last_error()
    assert L.i2r_conv_grouped(None, 1, None, 0, None) == E_ARG
