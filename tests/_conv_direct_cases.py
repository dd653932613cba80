"""Descriptors for the body / epilogue forms of the direct fp32 conv (csrc/i2r_conv.hip, conv_igemm_f32<MT, NT, CAP, PF, FORM, EPI>), built
on the Case class of _conv_cases.py: the smallest shapes that reach every path of conv_body_forms, each with the instantiation name and
the (form, epi) pair i2r_conv_direct_form must report for it.  tests/test_conv_direct_forms.py checks names and forms on the CPU,
tests/test_conv_direct_forms_gpu.py runs them.

Chunks (csrc/i2r_conv_plan.h, staging): a double-buffered member stages 12, 8 or 4 channel groups of 4 channels per chunk -- the largest
that divides cin / 4 and fits 2 * groups * plane * 16 bytes <= 40 KB, plane = patch pixels rounded up to 16.  So cin 48 is ONE chunk up to a
plane of 106 slots and three chunks of 16 channels above; cin 64 is two chunks of 32 up to 160 slots and four of 16 above; cin 96 two of 48.
A chunk of ck channels has taps * ck / 16 K steps: 27 | 18 | 9 for a 3x3 filter (the tail of the K loop takes 3 | 2 | 3 of them), 3 | 1 for a
1x1 filter with ck 48 | 16 (a chunk that is all tail | a single step).  A forced ck (i2r_conv_desc.ck) selects the synchronous variant PF 0."""
import ctypes as C

import _conv_cases as cc
from i2r_amd import cabi


def direct_form(descs):
    """(form, epi) of i2r_conv_direct_form for a list of descriptors; launches nothing"""
    arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
    f, e = C.c_int32(-1), C.c_int32(-1)
    cabi.check(cabi.lib().i2r_conv_direct_form(arr, len(descs), C.byref(f), C.byref(e)), "i2r_conv_direct_form")
    return f.value, e.value


def counts(members):
    """workgroups per member"""
    return [m.n * -(-m.conv_h // m.tile_h) * -(-m.conv_w // m.tile_w) * m.n_cblk for m in members]


def mk(tag, *, cin, cout, k, s, conv, tile, mt, wn, feature="relu", n=2, cout_pad=None, ck=0, parity=(0, 0), name=""):
    """one fp32 convolution: k x k filter (k = 2 with feature "deconv": the 2x2 taps of a transposed-conv output parity), stride s,
    conv map `conv`, tile `tile`; feature: relu | res1 | plain | in2 (+ res1) | up2 (rep 2 scatter onto res1 == out) | deconv"""
    cout_pad = cout_pad or cout
    c = cc.Case(name=name, tag=tag, dtype=0, feature=feature, mt=mt, wn=wn, tile_h=tile[0], tile_w=tile[1], ck=ck, in16=0, out16=0, n=n,
                cin=cin, cout_pad=cout_pad, cout=cout, stride=s, in2=False, nres=0, inplace=False, res_post=False, relu=1,
                out_step=1, out_off=(0, 0), rep=1)
    c.conv_h, c.conv_w = conv
    if feature == "deconv":
        assert k == 2 and s == 1
        c.taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
        c.iy0, c.ix0 = parity[0] - 1, parity[1] - 1
        c.in_h, c.in_w = conv
        c.out_step, c.out_off = 2, tuple(parity)
    else:
        c.taps = [(dy, dx) for dy in range(k) for dx in range(k)]
        c.iy0 = c.ix0 = -(k // 2)
        c.in_h, c.in_w = (conv if s == 1 else (2 * conv[0], 2 * conv[1]))
    if feature == "res1":
        c.nres = 1
    elif feature == "plain":
        c.relu = 0
    elif feature == "in2":
        c.in2, c.nres = True, 1
    elif feature == "up2":
        c.rep = c.out_step = 2
        c.nres, c.inplace = 1, True
    c.out_h, c.out_w = c.conv_h * c.out_step, c.conv_w * c.out_step
    c.in_cs, c.out_cs = cin, cout_pad
    c.n_cblk = cout_pad // 16 // (max(wn, 1) * next(x for x in cc.NTS if cout_pad // 16 % x == 0))
    return c


def _name(mt, nt, cap, pf):
    return cc.kernel_name(0, mt, nt, cap, pf)


# key: (case, instantiation, (form, epi))
SINGLES = {
    # one chunk: cin 48 -> 96, 3x3 stride 2, 16 x 12 -> 8 x 6 (tiles of 4 x 4: the second column of tiles is partial)
    "single-res1": (mk("s-res1", cin=48, cout=96, k=3, s=2, conv=(8, 6), tile=(4, 4), mt=1, wn=2, feature="res1"), _name(1, 3, 12, 1), (1, 2)),
    "single-relu": (mk("s-relu", cin=48, cout=96, k=3, s=2, conv=(8, 6), tile=(4, 4), mt=1, wn=2), _name(1, 3, 12, 1), (1, 1)),
    "single-plain": (mk("s-plain", cin=48, cout=96, k=3, s=2, conv=(8, 6), tile=(4, 4), mt=1, wn=2, feature="plain"), _name(1, 3, 12, 1), (1, 0)),
    # two chunks of 48: cin 96 -> 192, stride 2, ragged 10 x 7 map under 3 x 4 tiles (partial tiles, 12 pixels of a 16-pixel M fragment)
    "two-chunks-ragged": (mk("c2", cin=96, cout=192, k=3, s=2, conv=(10, 7), tile=(3, 4), mt=1, wn=4, feature="res1", n=1), _name(1, 3, 12, 1), (2, 2)),
    "two-chunks-in2": (mk("c2-in2", cin=96, cout=192, k=3, s=2, conv=(10, 7), tile=(3, 4), mt=1, wn=4, feature="in2", n=1), _name(1, 3, 12, 1), (0, 0)),
    # chunks of 16 channels: three (cin 48) and four (cin 64), stride 1 and 2; MT 2 and 3, NT 4
    "three-chunks-s1": (mk("c3s1", cin=48, cout=48, k=3, s=1, conv=(12, 13), tile=(8, 12), mt=2, wn=1, n=1), _name(2, 3, 4, 1), (2, 1)),
    "three-chunks-s2": (mk("c3s2", cin=48, cout=48, k=3, s=2, conv=(6, 10), tile=(4, 8), mt=1, wn=1, feature="res1", n=1), _name(1, 3, 4, 1), (2, 2)),
    "four-chunks-s1": (mk("c4s1", cin=64, cout=64, k=3, s=1, conv=(13, 14), tile=(12, 12), mt=3, wn=1, feature="res1", n=1), _name(3, 4, 4, 1), (2, 2)),
    "four-chunks-s2": (mk("c4s2", cin=64, cout=64, k=3, s=2, conv=(8, 11), tile=(6, 8), mt=1, wn=1, n=1), _name(1, 4, 4, 1), (2, 1)),
    # ... and with ck FORCED to 16: the synchronous variant, which the switch leaves alone
    "ck16-forced-s1": (mk("f3s1", cin=48, cout=48, k=3, s=1, conv=(6, 7), tile=(4, 4), mt=1, wn=1, ck=16, n=1), _name(1, 3, 4, 0), (0, 0)),
    "ck16-forced-s2": (mk("f4s2", cin=64, cout=64, k=3, s=2, conv=(6, 7), tile=(4, 4), mt=1, wn=1, ck=16, feature="res1", n=1), _name(1, 4, 4, 0), (0, 0)),
    # PF 2: an 8 x 8 tile at stride 2 has a 17 x 17 patch; three chunks, and one (cin 16)
    "pf2": (mk("pf2", cin=48, cout=48, k=3, s=2, conv=(10, 12), tile=(8, 8), mt=1, wn=1, feature="res1", n=1), _name(1, 3, 4, 2), (2, 2)),
    "pf2-single": (mk("pf2s", cin=16, cout=48, k=3, s=2, conv=(10, 12), tile=(8, 8), mt=1, wn=1, n=1), _name(1, 3, 4, 2), (1, 1)),
    # NT 5 (80 channels) with MT 2; a padded tail block (90 of 96 channels): the general epilogue under the single-chunk body
    "nt5-mt2": (mk("nt5", cin=48, cout=80, k=3, s=1, conv=(10, 13), tile=(8, 10), mt=2, wn=1, n=1), _name(2, 5, 4, 1), (2, 1)),
    "padded-cout": (mk("pad", cin=48, cout=90, cout_pad=96, k=3, s=2, conv=(8, 6), tile=(4, 4), mt=1, wn=2, feature="res1"), _name(1, 3, 12, 1), (1, 0)),
    # 1 x 1: a chunk that is all tail (3 steps, MT 2), chunks of a single step, the up-sampling scatter onto res1 == out
    "1x1-single-mt2": (mk("p1", cin=48, cout=48, k=1, s=1, conv=(10, 15), tile=(8, 12), mt=2, wn=1, n=1), _name(2, 3, 12, 1), (1, 1)),
    "1x1-single-res1": (mk("p1r", cin=48, cout=48, k=1, s=1, conv=(6, 5), tile=(6, 5), mt=1, wn=1, feature="res1"), _name(1, 3, 12, 1), (1, 2)),
    "1x1-one-step-chunks": (mk("p1c", cin=48, cout=48, k=1, s=1, conv=(18, 9), tile=(16, 8), mt=2, wn=1, feature="res1", n=1), _name(2, 3, 4, 1), (2, 2)),
    "1x1-up2-inplace": (mk("up2", cin=96, cout=48, k=1, s=1, conv=(6, 5), tile=(6, 5), mt=1, wn=1, feature="up2"), _name(1, 3, 12, 1), (2, 0)),
    # transposed-conv output parity (1, 0): 2 x 2 taps, results interleaved at step 2
    "deconv": (mk("dc", cin=48, cout=48, k=2, s=1, conv=(7, 6), tile=(4, 4), mt=1, wn=1, feature="deconv", parity=(1, 0)), _name(1, 3, 12, 1), (1, 1)),
}


def _fuse_down(tag, cin, feature, cout=96, wn=2):
    return mk(tag, cin=cin, cout=cout, k=3, s=2, conv=(8, 6), tile=(4, 4), mt=1, wn=wn, feature=feature, n=1)


# key: (members, instantiation, (form, epi)): three members with different K
GROUPS = {
    # 1, 2 and 4 chunks: the pipelined body for all
    "mixed-chunks": ([_fuse_down("g48", 48, "res1"), _fuse_down("g96", 96, "res1"), _fuse_down("g192", 192, "res1")], _name(1, 3, 12, 1), (2, 2)),
    # every member one chunk (27, 3 and 9 K steps): the single-chunk body
    "single-chunks": ([_fuse_down("h48", 48, "relu"), mk("h1", cin=48, cout=48, k=1, s=1, conv=(6, 5), tile=(4, 4), mt=1, wn=1, n=1),
                       _fuse_down("h16", 16, "relu", cout=48, wn=1)], _name(1, 3, 12, 1), (1, 1)),
    # the members disagree on res1: the general epilogue
    "mixed-res1": ([_fuse_down("m48", 48, "res1"), _fuse_down("m96", 96, "relu"), _fuse_down("m192", 192, "res1")], _name(1, 3, 12, 1), (2, 0)),
}

for _c, _n, _ in SINGLES.values():
    _c.name = _n
for _ms, _n, _ in GROUPS.values():
    for _m in _ms:
        _m.name = _n
