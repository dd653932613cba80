"""The static load / wait schedule of the Winograd pass loop (tools/wino_sched.py on csrc/i2r_conv_wino.hip; CPU, needs hipcc).

COVER of a load = MFMAs between its issue and the first s_waitcnt that forces its completion (in-order vmcnt model, see the tool).
A position of conv_wino_f32<1, 3> is 12 MFMAs, a pass 48.

Plain form conv_wino_f32<1, 3, 0 / 1 / 2>, the explicit schedule (WINO_PASS):
                          least cover of a weight load | of an activation (patch) load | vmcnt(0) before the staging store
    further pass   now        12                            24                              0
                   parent      1                            12                              1     (profiles/wino_sched_parent.json)
    first pass     now        12                            24                              0
                   parent      1                             1                              1
    last / only pass (no parent counterpart: `more` was a run-time flag):  weights 12.
Fused-input form conv_wino_fin_f32<1, 3, *>: KEEPS THE PARENT'S SCHEDULE (the explicit one spilled 26 registers at the 128 of 4 waves
per SIMD); its figures are asserted equal to the parent's table, so a change of either kind is noticed:
    further pass:  weights 0, activations 1, two vmcnt(0);   first pass:  weights 0, activations 0, one vmcnt(0).
Registers (from .amdhsa): <1, 3> at most 128 and no scratch (4 waves per SIMD); <1, 4> at most 168 and no scratch (3 waves per SIMD)."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="hipcc is not installed")

FORMS = (0, 1, 2)
PLAIN = ["conv_wino_f32<1, 3, %d>" % f for f in FORMS]
FUSED = ["conv_wino_fin_f32<1, 3, %d>" % f for f in FORMS]


@pytest.fixture(scope="session")
def table():
    import wino_sched
    return wino_sched.table()


@pytest.fixture(scope="session")
def parent():
    return json.load(open(os.path.join(ROOT, "profiles", "wino_sched_parent.json")))


def _show(name, kind, r):
    print("%s %s: %d MFMAs; weights %d loads, least cover %s; activations %d loads, least cover %s; vmcnt(0) %d (%d before the staging store)" % (
        name, kind, r["mfma"], r["n"]["weight"], r["min_cover"]["weight"], r["n"]["activation"], r["min_cover"]["activation"],
        r["vmcnt0"], r["vmcnt0_before_staging_store"]))


@pytest.mark.parametrize("name", PLAIN)
@pytest.mark.parametrize("kind", ["further", "first"])
def test_plain_form_passes_that_stage_a_chunk(table, name, kind):
    r = table[name]["regions"][kind]
    _show(name, kind, r)
    assert r["mfma"] == 48 and r["n"]["weight"] == 12 and r["n"]["activation"] == 2, "not the pass this check was written for"
    assert all(x["cover"] is not None for x in r["loads"])
    assert r["min_cover"]["weight"] >= 12
    assert r["min_cover"]["activation"] >= 24
    assert r["vmcnt0_before_staging_store"] == 0


@pytest.mark.parametrize("name", PLAIN)
@pytest.mark.parametrize("kind", ["last", "only"])
def test_plain_form_passes_without_a_next_chunk(table, name, kind):
    r = table[name]["regions"][kind]
    _show(name, kind, r)
    assert r["mfma"] == 48 and r["n"]["weight"] == 9 and r["n"]["activation"] == 0
    assert r["min_cover"]["weight"] >= 12


@pytest.mark.parametrize("name", PLAIN)
def test_parent_table_shows_what_the_schedule_removes(parent, name):
    """the committed `before`: weight loads with 1-2 MFMAs of cover, patch loads covered after about 12, vmcnt(0) inside position 3"""
    r = parent[name]["regions"]["further"]
    assert r["min_cover"]["weight"] <= 2 and r["min_cover"]["activation"] <= 12 and r["vmcnt0_before_staging_store"] >= 1


@pytest.mark.parametrize("name", FUSED)
def test_fused_input_form_keeps_the_parents_schedule(table, parent, name):
    assert sorted(table[name]["regions"]) == sorted(parent[name]["regions"]) == ["first", "further"]
    for kind in ("first", "further"):
        r, p = table[name]["regions"][kind], parent[name]["regions"][kind]
        _show(name, kind, r)
        assert r["min_cover"] == p["min_cover"] and r["n"] == p["n"]
        assert (r["vmcnt0"], r["vmcnt0_before_staging_store"]) == (p["vmcnt0"], p["vmcnt0_before_staging_store"])
    f, g = parent[name]["regions"]["further"], parent[name]["regions"]["first"]
    assert (f["min_cover"]["weight"], f["min_cover"]["activation"], f["vmcnt0_before_staging_store"]) == (0, 1, 2)
    assert (g["min_cover"]["weight"], g["min_cover"]["activation"], g["vmcnt0_before_staging_store"]) == (0, 0, 1)


def test_registers_and_scratch(table):
    assert len(table) == 12
    for name, k in table.items():
        print("%s: %d VGPRs, scratch %d" % (name, k["vgpr"], k["scratch"]))
        assert k["scratch"] == 0, name
        assert k["vgpr"] <= (128 if "<1, 3," in name else 168), name  # 512 registers per SIMD lane: 4 and 3 waves
