"""The static load / wait schedule of the direct fp32 conv's K loop (tools/conv_sched.py on csrc/i2r_conv.hip; CPU, needs hipcc).

For every instantiation conv_igemm_f32<MT, NT, CAP, PF, FORM, EPI> the flagship tower launches (names and forms asked from the engine's
own program at 16 crops, as tests/test_conv_dispatch.py does) plus the single-chunk forms of <1, 3, 12, 1>:
  * every weight load issued between MFMAs has at least one whole K step (4 MT NT MFMAs) of cover (the first step's weights of a chunk
    are issued ahead of the staging store and the barrier, outside the K blocks);
  * in a chunk that stages a successor no wait forces a patch load before the staging store, and there is no vmcnt(0);
  * no scalar load inside the chunk loop (FORM 2: up to the end of the chunk that stages a successor; with an epilogue form, EPI 1 | 2, none up
    to the last MFMA -- the general epilogue, EPI 0, reads its fields where the compiler puts them, behind the pass loop);
  * registers as recorded in profiles/conv_sched.json, no scratch; the single-chunk forms of <1, 3, 12, 1> fit 128 registers.
COVER = MFMAs between a load's issue and the first wait that forces it (in-order vmcnt model, see the tool)."""
import json
import os
import re
import shutil
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _conv_cases as cc  # noqa: E402
import _conv_direct_cases as dc  # noqa: E402
from i2r_amd import arch, cabi, config, engine, synth  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is not installed")

SINGLE_CHUNK = [(1, 3, 12, 1, 1, e) for e in (0, 1, 2)]


def flagship_forms():
    """(MT, NT, CAP, PF, FORM, EPI) of every direct fp32 launch of the w48 tower at 16 crops of 256 x 192 (a bench step runs two such programs)"""
    dev = torch.device("cpu")
    cfg = config.load_config("w48_pure_en6")
    pk = engine.Packer(synth.make_state_dict(arch.param_spec(cfg)), dev, "fp32")
    P = engine.Program(dev)
    P.store_dt = pk.dtype
    xs, _ = engine.HRNetW48(pk, "", cfg["MODEL"]["EXTRA"]).emit(P, 16, 256, 192)
    P.conv(xs[-1], pk.conv("reduce"), out_dt=0)
    out = set()
    cabi.lib().i2r_conv_direct_forms(1)
    for kind, _, st in P.ops:
        ds = [st] if kind == cabi.OP_CONV else [st.d[i].contents for i in range(st.n)] if kind == cabi.OP_CONV_GROUP else None
        if not ds or ds[0].algo == 1:
            continue
        rc, name, err = cc.resolve(ds)
        assert rc == 0, err
        out.add(tuple(int(x) for x in re.findall(r"\d+", name.split("<")[1])) + dc.direct_form(ds))
    return sorted(out)


@pytest.fixture(scope="session")
def forms():
    f = flagship_forms()
    assert len(f) >= 5 and all(t[3] > 0 and t[4] in (1, 2) for t in f), f  # (every direct conv of the tower is double-buffered and takes a form)
    return f


@pytest.fixture(scope="session")
def table(forms):
    import conv_sched
    return conv_sched.table(only=forms + SINGLE_CHUNK)


@pytest.fixture(scope="session")
def recorded():
    return json.load(open(os.path.join(ROOT, "profiles", "conv_sched.json")))


def _name(t):
    return "conv_igemm_f32<%d, %d, %d, %d, %d, %d>" % tuple(t)


def test_every_flagship_form_is_in_the_committed_table(forms, recorded):
    assert {_name(t) for t in forms + SINGLE_CHUNK} <= set(recorded), sorted({_name(t) for t in forms} - set(recorded))


def test_weight_loads_have_a_whole_k_step_of_cover(forms, table):
    for t in forms + SINGLE_CHUNK:
        k, step = table[_name(t)], 4 * t[0] * t[1]
        assert len(k["k_blocks"]) == (8 if t[4] == 2 else 4), (_name(t), len(k["k_blocks"]))
        n = 0
        for kb in k["k_blocks"]:
            print("%s %s: %d MFMAs, weights %d (least cover %s), other loads %d (least cover %s)" % (
                _name(t), kb["label"], kb["mfma"], kb["n"]["weight"], kb["least_cover"]["weight"], kb["n"]["activation"], kb["least_cover"]["activation"]))
            if kb["n"]["weight"]:
                assert kb["least_cover"]["weight"] >= step, (_name(t), kb["label"])
            n += kb["n"]["weight"]
        assert n >= 3 * t[1], _name(t)  # (loop: two steps; tails: two and one)


def test_no_wait_forces_the_next_chunks_patch_before_its_staging_store(forms, table):
    for t in forms:
        if t[4] != 2:
            continue
        staging = table[_name(t)]["k_blocks"][:4]  # the chunk with a successor: loop and three tails
        assert [kb["loop"] for kb in staging] == [True, False, False, False], _name(t)
        assert sum(kb["n"]["activation"] for kb in staging[1:]) == 3 * (t[2] // 4) * 4 * t[3], _name(t)  # CAP / 4 x 4 PF patch loads in each tail
        for kb in staging:
            assert kb["activation_forced_in_block"] == 0 and kb["vmcnt0"] == 0, (_name(t), kb["label"])
            if kb["n"]["activation"]:
                assert kb["least_cover"]["activation"] >= min(kb["mfma"], 8 * t[0] * t[1]), (_name(t), kb["label"])  # two K steps; one in a one-step chunk


def test_no_scalar_load_inside_the_chunk_loop(forms, table):
    for t in forms + SINGLE_CHUNK:
        kbs = table[_name(t)]["k_blocks"]
        inside = kbs[1:4] if t[4] == 2 else []
        if t[5] != 0:
            inside = kbs[1:]
        assert sum(kb["smem_since_previous_k_block"] for kb in inside) == 0, _name(t)


def test_registers_and_scratch_are_as_recorded(forms, table, recorded):
    for t in forms + SINGLE_CHUNK:
        k, r = table[_name(t)], recorded[_name(t)]
        print("%s: %d VGPRs, scratch %d" % (_name(t), k["vgpr"], k["scratch"]))
        assert k["scratch"] == 0 and k["vgpr"] == r["vgpr"], (_name(t), k["vgpr"], r["vgpr"])
    for t in SINGLE_CHUNK:
        assert table[_name(t)]["vgpr"] <= 128, _name(t)  # four waves per SIMD
