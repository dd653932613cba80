"""CPU: runs of fragments in the Winograd kernels (i2r_conv_desc.seq, csrc/i2r_conv_wino.hip) -- the descriptor field, what the library
resolves when it chooses (i2r_conv_grid launches nothing) and the workgroup floor its rule states."""
import ctypes as C
import os
import subprocess

import pytest

import _conv_cases as cc
from i2r_amd import cabi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1  # I2R_E_ARG of include/i2r_hip.h
TAPS = [(t // 3, t % 3) for t in range(9)]
# the rule's own constants (wino_choose_seq in csrc/i2r_conv_plan.h): a launch the library sizes keeps min(what it had at one fragment per
# workgroup, MIN_WG) workgroups and fills its runs up to RUN_PASSES 16-channel passes, 8 fragments at the most
MIN_WG, RUN_PASSES, MAX_SEQ = 512, 6, 8


def wino_desc(n, c, h, w, seq=0, cout=None, out=0x40000):
    cout = cout or c
    fw, fh = engine.wino_fragment(h, w)
    return cc.make_desc(n_img=n, in_h=h, in_w=w, in_cs=c, cin=c, conv_h=h, conv_w=w, out_h=h, out_w=w, out_cs=cout, cout=cout, cout_pad=cout,
                        stride=1, iy0=-1, ix0=-1, taps=TAPS, tile_h=fh, tile_w=fw, mt=1, wn=1, relu=1, algo=1, out=out), seq


def grid(members, with_map):
    """-> (rc, workgroups, run length per member) of i2r_conv_grid"""
    descs = []
    for d, seq in members:
        d.seq = seq
        descs.append(d)
    arr = (C.POINTER(cabi.ConvDesc) * len(descs))(*[C.pointer(d) for d in descs])
    g, seqs = C.c_int32(-1), (C.c_int32 * len(descs))()
    rc = cabi.lib().i2r_conv_grid(arr, len(descs), int(with_map), C.byref(g), seqs)
    return rc, g.value, list(seqs)


def fragments(n, h, w):
    fw, fh = engine.wino_fragment(h, w)
    return n * -(-h // fh) * -(-w // fw)


@pytest.mark.parametrize("seq", [-1, 9, 100])
def test_seq_outside_its_range_is_rejected(seq):
    rc, _, _ = grid([wino_desc(2, 48, 16, 12, seq)], True)
    assert rc == E_ARG and b"seq=%d" % seq in cabi.lib().i2r_last_error()
    d, _ = wino_desc(2, 48, 16, 12)
    d.seq = seq
    assert cc.resolve([d])[0] == E_ARG
    assert cabi.lib().i2r_conv(C.byref(d), None) == E_ARG  # (refused before the device is touched)


@pytest.mark.parametrize("seq", range(1, 9))
def test_forced_seq_divides_the_fragments_into_runs(seq):
    """3 crops of 16x12 (3 fragments each, 9 in all), 48 -> 96 (two channel blocks): runs with a table, whole rounds of 8 runs without"""
    m = wino_desc(3, 48, 16, 12, seq, cout=96)
    assert fragments(3, 16, 12) == 9
    runs = -(-9 // seq)
    assert grid([m], True) == (0, runs * 2, [seq])
    assert grid([m], False) == (0, -(-runs // 8) * 8 * 2, [seq])


def test_a_lone_192_channel_member_runs_one_fragment_per_workgroup():
    for n in (1, 2, 16, 32):
        rc, g, seqs = grid([wino_desc(n, 192, 16, 12)], True)
        assert (rc, seqs) == (0, [1]) and g == fragments(n, 16, 12) * 4


def _stage3(n):
    return [wino_desc(n, 192, 16, 12, out=0x40000), wino_desc(n, 96, 32, 24, out=0x50000), wino_desc(n, 48, 64, 48, out=0x60000)]


GROUPS = ([("stage3-%d" % n, _stage3(n)) for n in (1, 2, 3, 8, 16, 32)] + [("stage2-%d" % n, _stage3(n)[1:]) for n in (2, 16, 32)] +
          [("lone48-%d" % n, [wino_desc(n, 48, 64, 48)]) for n in (1, 2, 5, 16, 32)] + [("layer1-%d" % n, [wino_desc(n, 64, 64, 48)]) for n in (2, 16, 32)] +
          [("one-pass-%d" % n, [wino_desc(n, 16, 64, 48, cout=48)]) for n in (4, 32)])


@pytest.mark.parametrize("members", [g[1] for g in GROUPS], ids=[g[0] for g in GROUPS])
def test_the_librarys_choice_keeps_the_workgroup_floor(members):
    rc1, at_one, _ = grid([(d, 1) for d, _ in members], True)
    rc0, chosen, seqs = grid([(d, 0) for d, _ in members], True)
    assert rc1 == 0 and rc0 == 0
    assert chosen >= min(at_one, MIN_WG), (chosen, at_one, seqs)
    for (d, _), s in zip(members, seqs):
        assert 1 <= s <= MAX_SEQ and s * (d.cin // 16) <= max(RUN_PASSES, d.cin // 16), (d.cin, s)
    # forcing what the library chose gives the same grid, banded or not
    for with_map in (True, False):
        assert grid([(d, s) for (d, _), s in zip(members, seqs)], with_map)[1] == grid([(d, 0) for d, _ in members], with_map)[1]


@pytest.mark.parametrize("n", [16, 32])
def test_stage3_pairs_its_48_channel_fragments(n):
    """the launch the flagship workload spends its time in: 192 / 96 / 48 channels resolve to 1 / 1 / 2 (runs of up to RUN_PASSES passes)"""
    rc, g, seqs = grid(_stage3(n), True)
    assert (rc, seqs) == (0, [1, 1, 2])
    assert g == n * (3 * 4 + 12 * 2 + 24) and g >= MIN_WG  # 192: 3 fragments x 4 blocks, 96: 12 x 2, 48: 48 fragments in 24 runs


def test_the_floor_takes_runs_back_from_a_small_launch():
    """stage 3 needs 9 crops to keep MIN_WG workgroups with paired 48-channel fragments (60 per crop); one-pass items (16 channels, 48
    fragments per crop) would run six to a workgroup: at 32 crops the floor leaves them three (1536 / 3 = 512), at 4 crops one"""
    assert grid(_stage3(8), True)[2] == [1, 1, 1] and grid(_stage3(9), True)[2] == [1, 1, 2]
    rc, g, seqs = grid([wino_desc(32, 16, 64, 48, cout=48)], True)
    assert (rc, seqs, g) == (0, [3], MIN_WG) and 32 * 48 // 4 < MIN_WG
    assert grid([wino_desc(4, 16, 64, 48, cout=48)], True)[2] == [1]


def test_a_forced_member_keeps_its_run_length_beside_chosen_ones():
    ms = _stage3(32)
    rc, g, seqs = grid([ms[0], (ms[1][0], 1), ms[2]], True)
    assert rc == 0 and seqs[1] == 1 and seqs[0] == 1 and g >= MIN_WG


def test_engine_constant_passes_zero_or_one():
    import torch
    from i2r_amd import synth
    sd = {"c.weight": torch.from_numpy(synth._sym(1, "w", (48, 48, 3, 3), 0.05))}
    pc = engine.Packer(sd, torch.device("cpu")).conv("c", None)
    saved = engine.WINO_SEQ
    try:
        for on in (True, False):
            engine.WINO_SEQ = on
            P = engine.Program(torch.device("cpu"))
            P.conv(P.alloc(2, 16, 12, 48), pc, relu=True)
            (st,) = [st for k, _, st in P.ops if k == cabi.OP_CONV_GROUP]
            assert st.d[0].contents.algo == 1 and st.d[0].contents.seq == (0 if on else 1)
    finally:
        engine.WINO_SEQ = saved


def test_conv_desc_mirror_matches_the_header(tmp_path):
    """sizeof, and the offsets of the last pointer and of seq behind it, of the ctypes mirror equal the C struct's (a tiny gcc program)"""
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "i2r_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(i2r_conv_desc), offsetof(i2r_conv_desc, y), offsetof(i2r_conv_desc, seq)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(cabi.ConvDesc), cabi.ConvDesc.y.offset, cabi.ConvDesc.seq.offset]
    assert cabi.ConvDesc._fields_[-1][0] == "seq" and "i2r_conv_grid" in cabi.EXPORTS
