"""CPU: validation loss + PCK accuracy + target heat maps -- the numpy restatement tests/_val_ref.py against the reference's own output
(tests/golden/val_metrics_reference.npz, written by tools/make_golden_val_metrics.py from generate_target / JointsMSELoss / accuracy), the
fixture's recorded conditions, and the C-ABI surface of i2r_joint_targets / i2r_val_metrics."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import _val_ref
from i2r_amd import cabi, caller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "val_metrics_reference.npz")
CASES = [(1, 1, 7, 5), (1, 17, 16, 12), (5, 17, 20, 20), (3, 14, 17, 13), (2, 14, 64, 48)]
_CACHE = {}


def fixture():
    if "f" not in _CACHE:
        with np.load(FIX) as f:
            _CACHE["f"] = {k: f[k] for k in f.files}
    return _CACHE["f"]


def case(ci):
    """-> namespace of case ci: inputs, the reference's outputs, the recorded margins (arrays are shared: do not write to them)"""
    if ci not in _CACHE:
        f = fixture()
        d = types.SimpleNamespace(**{k[len("c%d_" % ci):]: v for k, v in f.items() if k.startswith("c%d_" % ci)})
        d.S, d.J, d.h, d.w = (int(v) for v in f["cases"][ci])
        d.sigma = int(f["sigma"])
        d.jw = d.joints_weight if d.joints_weight.size else None
        for a in vars(d).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[ci] = d
    return _CACHE[ci]


def restated(ci, use_w):
    """_val_ref on the fixture's output and the REFERENCE's target (computed once per case and flag)"""
    key = ("ref", ci, use_w)
    if key not in _CACHE:
        d = case(ci)
        _CACHE[key] = _val_ref.val_metrics(d.output, d.target, d.target_weight, bool(use_w))
    return _CACHE[key]


def test_fixture_holds_the_cases_of_the_issue():
    f = fixture()
    assert [tuple(int(v) for v in c) for c in f["cases"]] == CASES and int(f["sigma"]) == 2
    assert os.path.getsize(FIX) < 1 << 20
    assert int(str(f["numpy_version"]).split(".")[0]) >= 2, "generate_target's float32 - float64 promotes to float64 under NumPy 2"
    undrawn = [((case(ci).joints_vis == 0.5) & (case(ci).target_weight > 0) & (case(ci).target == 0).all((2, 3))).sum() for ci in range(len(CASES))]
    assert sum(undrawn) > 0, "the fixture holds joints that are not drawn but weighted (visibility 0.5)"


def _c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        base = re.match(r"(const\s+)?(\w+)", decl).group(2)
        for part in decl[re.match(r"(const\s+)?\w+", decl).end():].split(","):
            ptr = "*" in part
            out.append((part.replace("*", "").strip(), ctypes.c_void_p if ptr else {"double": ctypes.c_double, "int32_t": ctypes.c_int32}[base]))
    return out


def test_header_binding_and_exports_agree_and_abi_stays_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    for sym, struct, cls in (("i2r_joint_targets", "i2r_joint_targets_args", cabi.JointTargetsArgs),
                             ("i2r_val_metrics", "i2r_val_metrics_args", cabi.ValMetricsArgs)):
        assert re.search(r"^I2R_API\s+int\s+%s\s*\(const %s\* a, void\* stream\);" % (sym, struct), header, flags=re.M)
        assert sym in cabi.EXPORTS
        assert _c_struct_fields(header, struct) == [(n, t) for n, t in cls._fields_], struct
    assert ctypes.sizeof(cabi.JointTargetsArgs) == 5 * 8 + 8 + 4 * 4 and ctypes.sizeof(cabi.ValMetricsArgs) == 16 * 8 + 8 + 6 * 4
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    exported = __graft_entry__.exported_symbols(cabi.LIB_PATH)
    assert "i2r_joint_targets" in exported and "i2r_val_metrics" in exported
    assert "i2r_metrics.hip" in __graft_entry__.SOURCES


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_restatement_reproduces_the_reference(ci):
    d = case(ci)
    target, tw = _val_ref.joint_targets(d.joints_hm, d.joints_vis, d.h, d.w, d.sigma, d.jw)
    assert np.array_equal(tw, d.target_weight)
    err = float(np.abs(target.astype(np.float64) - d.target).max())
    print("case %d: target max-abs vs the reference %.3g" % (ci, err))
    assert err <= 6e-8                                            # 1 fp32 ulp below 1
    assert np.array_equal(target == 0, d.target == 0)
    for use_w in (1, 0):
        r = restated(ci, use_w)
        assert np.array_equal(r.acc, d.acc) and r.avg_acc == float(d.avg_acc) and r.cnt == int(d.cnt)
        assert np.array_equal(r.pred, d.pred) and r.pred.dtype == d.pred.dtype == np.float32
        recorded = float(getattr(d, "loss_rel_w%d" % use_w))
        ref32 = float(getattr(d, "loss_w%d" % use_w))
        print("case %d use_w %d: reference fp32 loss %.9g, float64 sum %.17g, recorded distance %.3g" % (ci, use_w, ref32, r.loss, recorded))
        assert recorded <= 1e-6
        assert abs(r.loss - ref32) <= (recorded + 1.2e-10) * r.loss   # (+ the order of the float64 sum: 2^20 * 2^-53)
        assert abs(r.loss - float(getattr(d, "loss64_w%d" % use_w))) <= 1.2e-10 * r.loss


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_fixture_meets_its_recorded_conditions(ci):
    d = case(ci)
    f = fixture()
    mu = d.joints_hm
    frac = float(np.abs(mu - np.floor(mu) - 0.5).min())
    assert frac >= float(f["frac_margin_required"]) == 1e-3 and abs(frac - float(d.min_frac_margin)) < 1e-12            # (a)
    dists = []
    r = _val_ref.val_metrics(d.output, d.target, d.target_weight, True, dists_out=dists)
    margin = float(np.abs(np.asarray(dists) - 0.5).min())
    assert margin >= float(f["dist_margin_required"]) == 1e-6 and abs(margin - float(d.min_dist_margin)) < 1e-9          # (b)
    hits, counted, total = int(r.hits.sum()), int(r.valid.sum()), d.S * d.J
    n_zero = int((d.target_weight == 0).sum())
    if total == 1:
        # a case of one map can be only one of hit / miss / ignored / zero-weight: it is a counted joint and a hit
        assert (hits, counted, n_zero) == (1, 1, 0)
        return
    assert hits > 0 and counted - hits > 0 and total - counted > 0 and n_zero > 0
    # the planted joints: on both sides of each of the four cut-offs, in the order the generator documents
    w, h = d.w, d.h
    want_mu = [(-8.0, None), (-7.999, None), (w + 6.0, None), (w + 5.999, None), (None, -8.0), (None, -7.999), (None, h + 6.0), (None, h + 5.999)]
    assert d.plants.shape == (8, 2)
    for k, ((s, j), (mx, my)) in enumerate(zip(d.plants, want_mu)):
        assert (mx is None or mu[s, j, 0] == mx) and (my is None or mu[s, j, 1] == my) and d.joints_vis[s, j] == 1
        jw = 1.0 if d.jw is None else float(d.jw[j])
        assert d.target_weight[s, j] == (0.0 if k % 2 == 0 else np.float32(jw)), (k, s, j)
        assert (d.target[s, j] != 0).any() == (k % 2 == 1)
    assert (d.jw is not None) == (ci == 2)


def test_heatmap_joints_and_config_tables():
    """host side of the caller: image-space joints -> heat-map coordinates through input.affine_transforms (float64), and the tables"""
    from i2r_amd import config, input as i2r_input
    center, scale = np.array([[320.0, 240.0], [100.5, 90.25]]), np.array([[1.2, 1.6], [0.6, 0.8]])
    joints = np.array([[[320.0, 240.0], [200.0, 100.0]], [[100.5, 90.25], [10.0, 20.0]]])
    hm = caller.heatmap_joints(joints, center, scale, (48, 64))
    assert hm.dtype == np.float64 and hm.shape == (2, 2, 2)
    assert np.allclose(hm[:, 0], [[23.5, 31.5]] * 2, atol=1e-9), "the crop centre lands on the centre of the map"
    t = i2r_input.affine_transforms(center, scale, (48, 64))
    assert np.allclose(hm[1, 1], np.dot(t[1], np.array([10.0, 20.0, 1.0])), rtol=1e-13, atol=0)   # affine_transform, transforms.py:93-96
    assert sorted(caller.JOINTS_WEIGHT) == sorted(caller.FLIP_PAIRS)
    assert len(caller.JOINTS_WEIGHT["coco"]) == 17 == len(caller.JOINTS_WEIGHT["ochuman"]) and len(caller.JOINTS_WEIGHT["crowdpose"]) == 14
    assert np.array_equal(np.asarray(caller.JOINTS_WEIGHT["coco"], np.float32), case(2).joints_weight)
    cfg = config.load_config("w48_pure_en6", ["LOSS.USE_OHKM", "True"])
    with pytest.raises(cabi.I2RError, match="OHKM"):
        caller.val_metrics_cfg(cfg, None)
