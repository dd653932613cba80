"""-m gpu: i2r_joint_targets and i2r_val_metrics (validation loss + PCK accuracy on the device) through the raw C-ABI, with canaries around
every output: against the reference's own output (tests/golden/val_metrics_reference.npz), against the numpy restatement tests/_val_ref.py
for constructed inputs, the ValMeter arithmetic, and end to end behind the model."""
import ctypes

import numpy as np
import pytest
import torch

import _val_ref
from _golden import setup
from i2r_amd import cabi, caller, models
from test_val_metrics import CASES, case, restated

pytestmark = pytest.mark.gpu

GUARD = 64          # canary elements on either side of every output
CANARY = {torch.float64: -12345.5, torch.float32: -4321.25, torch.int32: -77}
DELTA = 2.5e-7      # the bound on |device target - reference target|: 4 fp32 ulp at 1
SUM_RTOL = 1.2e-10  # 2^20 * 2^-53: the worst case of an fp64 sum of up to 2^20 terms


def dev():
    return torch.device("cuda", 0)


def up(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(dev())     # (a copy: the fixture's arrays are read-only)


class Guarded:
    """an output buffer of n elements between two rows of canaries"""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.t = torch.full((n + 2 * GUARD,), CANARY[dtype], dtype=dtype, device=dev())

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def get(self):
        """-> numpy, canaries stripped AFTER checking them"""
        a = self.t.cpu().numpy()
        assert (a[:GUARD] == CANARY[self.dtype]).all() and (a[-GUARD:] == CANARY[self.dtype]).all(), "canary overwritten"
        return a[GUARD:-GUARD] if self.n else a[:0]

    def untouched(self):
        return bool((self.t.cpu().numpy() == CANARY[self.dtype]).all())


class Outs:
    NAMES = ("loss", "acc", "avg_acc", "sse", "cnt", "hits", "valid", "pred", "ws")

    def __init__(self, S, J):
        f64, i32 = torch.float64, torch.int32
        self.loss, self.acc, self.avg_acc, self.sse = Guarded(1, f64), Guarded(J + 1, f64), Guarded(1, f64), Guarded(J, f64)
        self.cnt, self.hits, self.valid = Guarded(1, i32), Guarded(J, i32), Guarded(J, i32)
        self.pred, self.ws = Guarded(S * J * 2, torch.float32), Guarded(2 * S * J, f64)

    def get(self, S, J):
        r = _val_ref.Result()
        for n in self.NAMES:
            setattr(r, n, getattr(self, n).get().copy())
        r.loss, r.avg_acc, r.cnt, r.pred = float(r.loss[0]), float(r.avg_acc[0]), int(r.cnt[0]), r.pred.reshape(S, J, 2)
        return r

    def untouched(self):
        return all(getattr(self, n).untouched() for n in self.NAMES)


def run_metrics(output, target=None, target_weight=None, joints_hm=None, joints_vis=None, joints_weight=None, sigma=2, use_w=True,
                meter=None, expect=0, out_offset=0, **kw):
    """the raw C-ABI call; output [S, J, h, w] numpy.  out_offset: floats by which the maps are shifted off their 16-byte boundary.
    -> (results with canaries checked | None when expect != 0, the Outs)"""
    S, J, h, w = output.shape
    keep = []

    def maps(a):
        t = torch.zeros(a.size + out_offset, dtype=torch.float32, device=dev())
        t[out_offset:] = up(a, np.float32).reshape(-1)
        keep.append(t)
        return t.data_ptr() + 4 * out_offset
    o = Outs(S, J)
    a = cabi.ValMetricsArgs(output=maps(output) if output.size else None, ws=o.ws.ptr(), loss=o.loss.ptr(), acc=o.acc.ptr(), avg_acc=o.avg_acc.ptr(),
                            cnt=o.cnt.ptr(), pred=o.pred.ptr(), sse=o.sse.ptr(), hits=o.hits.ptr(), valid=o.valid.ptr(), meter=meter,
                            sigma=float(sigma), n_crops=S, joints=J, h=h, w=w, use_target_weight=int(bool(use_w)))
    if target is not None:
        a.target = maps(target) if target.size else 8   # (never read when there is no crop)
    for name, v, dt in (("target_weight", target_weight, np.float32), ("joints_hm", joints_hm, np.float64), ("joints_vis", joints_vis, np.float32),
                        ("joints_weight", joints_weight, np.float32)):
        if v is not None:
            keep.append(up(v, dt))
            setattr(a, name, keep[-1].data_ptr() if keep[-1].numel() else 8)
    for k, v in kw.items():
        setattr(a, k, v)
    rc = cabi.lib().i2r_val_metrics(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    torch.cuda.synchronize()
    return (o.get(S, J) if expect == 0 and S > 0 else None), o


def run_targets(joints_hm, joints_vis, h, w, joints_weight=None, sigma=2, want_target=True, expect=0, kw=None):
    S, J = joints_hm.shape[:2]
    hm, vis = up(joints_hm, np.float64), up(joints_vis, np.float32)
    jw = up(joints_weight, np.float32) if joints_weight is not None else None
    tw, target = Guarded(S * J, torch.float32), Guarded(S * J * h * w, torch.float32)
    a = cabi.JointTargetsArgs(joints_hm=hm.data_ptr() if S else 8, joints_vis=vis.data_ptr() if S else 8, joints_weight=jw.data_ptr() if jw is not None else None,
                              target_weight=tw.ptr(), target=target.ptr() if want_target else None, sigma=float(sigma), n_crops=S, joints=J, h=h, w=w)
    for k, v in (kw or {}).items():      # fields overwritten after the fact: bad arguments
        setattr(a, k, v)
    rc = cabi.lib().i2r_joint_targets(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    torch.cuda.synchronize()
    return tw, target


def assert_discrete_equal(got, want, what=""):
    """everything that is decided, not summed: bit-identical"""
    assert np.array_equal(got.hits, want.hits) and np.array_equal(got.valid, want.valid), (what, got.hits, want.hits, got.valid, want.valid)
    assert np.array_equal(got.acc.view(np.uint64), np.asarray(want.acc, np.float64).view(np.uint64)), (what, got.acc, want.acc)
    assert np.float64(got.avg_acc).view(np.uint64) == np.float64(want.avg_acc).view(np.uint64) and got.cnt == int(want.cnt), what
    assert got.pred.dtype == np.float32 and np.array_equal(got.pred.view(np.uint32), np.asarray(want.pred, np.float32).view(np.uint32)), what


def assert_sums_close(got, want, what=""):
    rel = np.abs(got.sse - want.sse) / np.where(want.sse != 0, want.sse, 1.0)
    lrel = abs(got.loss - want.loss) / (want.loss if want.loss != 0 else 1.0)
    print("%s: sse max rel %.3g, loss rel %.3g (bound %.3g)" % (what, rel.max(), lrel, SUM_RTOL))
    assert (rel <= SUM_RTOL).all() and lrel <= SUM_RTOL, (what, rel.max(), lrel)


def analytic_loss_bound(output, target, tw, use_w):
    """0.5 / (J S h w) * sum w^2 (2 |p - t| delta + delta^2), in float64 from the reference target"""
    S, J, h, w = output.shape
    wt = np.asarray(tw, np.float64).reshape(S, J, 1, 1) if use_w else np.ones((S, J, 1, 1))
    d = np.abs(output.astype(np.float64) - target.astype(np.float64))
    return 0.5 / (J * S * h * w) * float((wt * wt * (2 * d * DELTA + DELTA * DELTA)).sum())


def check_tensor(output, target, tw, use_w=True, what="", **kw):
    want = _val_ref.val_metrics(output, target, tw, use_w)
    got, _ = run_metrics(output, target=target, target_weight=tw, use_w=use_w, **kw)
    assert_discrete_equal(got, want, what)
    assert_sums_close(got, want, what)
    return got, want


def check_analytic(output, mu, vis, use_w=True, jw=None, sigma=2, what="", **kw):
    S, J, h, w = output.shape
    target, tw = _val_ref.joint_targets(mu, vis, h, w, sigma, jw)
    want = _val_ref.val_metrics(output, target, tw, use_w)
    got, _ = run_metrics(output, joints_hm=mu, joints_vis=vis, joints_weight=jw, sigma=sigma, use_w=use_w, **kw)
    assert_discrete_equal(got, want, what)
    bound = analytic_loss_bound(output, target, tw, use_w)
    print("%s: analytic loss %.17g, restated %.17g, |diff| %.3g, bound %.3g" % (what, got.loss, want.loss, abs(got.loss - want.loss), bound))
    assert abs(got.loss - want.loss) <= bound, (what, got.loss, want.loss, bound)
    return got, want


# ---- against the reference's own output -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", range(len(CASES)))
def test_joint_targets_equal_the_reference(ci):
    """target_weight exact (the planted joints on both sides of every cut-off among them), target within 2.5e-7; a null target pointer
    writes only the weights"""
    d = case(ci)
    tw, target = run_targets(d.joints_hm, d.joints_vis, d.h, d.w, d.jw, d.sigma)
    got_w, got_t = tw.get().reshape(d.S, d.J), target.get().reshape(d.S, d.J, d.h, d.w)
    assert np.array_equal(got_w.view(np.uint32), d.target_weight.view(np.uint32))
    for k, (s, j) in enumerate(d.plants):
        assert (got_w[s, j] == 0) == (k % 2 == 0) and (got_t[s, j] != 0).any() == (k % 2 == 1), (k, s, j)
    err = float(np.abs(got_t.astype(np.float64) - d.target).max())
    print("case %d: target max-abs vs the reference %.3g (bound %.3g)" % (ci, err, DELTA))
    assert err <= DELTA
    drawn = (d.target != 0).any((2, 3))       # (per map: far tails below fp32's normal range may be flushed to zero by expf)
    assert np.array_equal((got_t != 0).any((2, 3)), drawn) and (got_t[~drawn] == 0).all(), "maps that are not drawn are zero everywhere"
    tw2, target2 = run_targets(d.joints_hm, d.joints_vis, d.h, d.w, d.jw, d.sigma, want_target=False)
    assert np.array_equal(tw2.get().view(np.uint32), d.target_weight.reshape(-1).view(np.uint32)) and target2.untouched()


@pytest.mark.parametrize("use_w", [1, 0])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_tensor_mode_equals_the_reference(ci, use_w):
    d = case(ci)
    want = restated(ci, use_w)      # float64 sums of the fp32 terms; its discrete outputs equal the reference's (test_val_metrics.py)
    got, _ = run_metrics(d.output, target=d.target, target_weight=d.target_weight, use_w=use_w)
    ref = _val_ref.Result()
    ref.acc, ref.avg_acc, ref.cnt, ref.pred, ref.hits, ref.valid = d.acc, float(d.avg_acc), int(d.cnt), d.pred, want.hits, want.valid
    assert_discrete_equal(got, ref, "case %d" % ci)
    assert_sums_close(got, want, "case %d use_w %d" % (ci, use_w))
    assert abs(got.loss - float(getattr(d, "loss64_w%d" % use_w))) <= SUM_RTOL * got.loss
    assert abs(got.loss - float(getattr(d, "loss_w%d" % use_w))) <= (float(getattr(d, "loss_rel_w%d" % use_w)) + SUM_RTOL) * got.loss


@pytest.mark.parametrize("use_w", [1, 0])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_analytic_mode_equals_the_reference(ci, use_w):
    d = case(ci)
    want = restated(ci, use_w)
    got, _ = run_metrics(d.output, joints_hm=d.joints_hm, joints_vis=d.joints_vis, joints_weight=d.jw, sigma=d.sigma, use_w=use_w)
    ref = _val_ref.Result()
    ref.acc, ref.avg_acc, ref.cnt, ref.pred, ref.hits, ref.valid = d.acc, float(d.avg_acc), int(d.cnt), d.pred, want.hits, want.valid
    assert_discrete_equal(got, ref, "case %d" % ci)
    bound = analytic_loss_bound(d.output, d.target, d.target_weight, use_w)
    print("case %d use_w %d: analytic loss %.17g, float64 %.17g, |diff| %.3g, bound %.3g" % (ci, use_w, got.loss, want.loss, abs(got.loss - want.loss), bound))
    assert abs(got.loss - want.loss) <= bound
    # through the Python surface: the same bits as the raw call
    jw = None if d.jw is None else d.jw.copy()
    m = caller.val_metrics(up(d.output, np.float32), joints_hm=d.joints_hm.copy(), joints_vis=d.joints_vis.copy(), sigma=d.sigma, joints_weight=jw,
                           use_target_weight=bool(use_w))
    assert m.loss.item() == got.loss and np.array_equal(m.acc.cpu().numpy(), got.acc) and m.cnt.item() == got.cnt
    assert np.array_equal(m.pred.cpu().numpy(), got.pred) and np.array_equal(m.sse.cpu().numpy(), got.sse)
    assert np.array_equal(m.hits.cpu().numpy(), got.hits) and np.array_equal(m.valid.cpu().numpy(), got.valid)
    t_dev, tw_dev = caller.joint_targets(d.joints_hm.copy(), d.joints_vis.copy(), (d.w, d.h), d.sigma, jw)
    m2 = caller.val_metrics(up(d.output, np.float32), t_dev, tw_dev, use_target_weight=bool(use_w))
    assert m2.loss.item() == pytest.approx(got.loss, rel=SUM_RTOL) and torch.equal(m2.acc, m.acc) and torch.equal(m2.pred, m.pred)


# ---- constructed inputs against the restatement ------------------------------------------------------------------------------------

def test_terms_are_the_separately_rounded_fp32_operations():
    """maps of ONE pixel: sse[j] is a single term, which must be the fp32 value ((p * w) - (t * w))^2 with four roundings -- bit for bit"""
    rng = np.random.default_rng(11)
    J = 500
    p, t = rng.standard_normal((1, J, 1, 1)).astype(np.float32), rng.standard_normal((1, J, 1, 1)).astype(np.float32)
    tw = rng.uniform(0.1, 1.9, (1, J)).astype(np.float32)
    for use_w in (1, 0):
        got, _ = run_metrics(p, target=t, target_weight=tw, use_w=use_w)
        want = _val_ref.sse_terms(p, t, tw, use_w).reshape(J)
        fused = ((p.astype(np.float64) * tw.reshape(1, J, 1, 1) - t.astype(np.float64) * tw.reshape(1, J, 1, 1)) ** 2).reshape(J)
        assert use_w == 0 or (want.astype(np.float64) != fused).any(), "the inputs tell separate roundings from a contracted form"
        assert np.array_equal(got.sse.view(np.uint64), want.astype(np.float64).view(np.uint64))


def _blank(S, J, h, w, fill=-0.25):
    return np.full((S, J, h, w), fill, np.float32)


def test_argmax_ties_and_non_positive_maps():
    S, J, h, w = 2, 3, 9, 11
    out = _blank(S, J, h, w)
    target = np.zeros((S, J, h, w), np.float32)
    target[:, :, 4, 5] = 1.0                                   # every joint counted: target peak (5, 4)
    out[0, 0, 6, 3] = out[0, 0, 2, 7] = 0.75                   # two equal maxima -> the first flat index: (7, 2)
    out[0, 1, 4, 5] = 0.5
    out[0, 2] = -1.0                                           # all negative -> (0, 0)
    out[1, 0] = 0.0                                            # all zero -> (0, 0): the maximum is not > 0
    out[1, 1, 8, 10] = 1e-30                                   # the last pixel, barely positive
    out[1, 2, 0, 0] = 3.0
    got, want = check_tensor(out, target, np.ones((S, J), np.float32), what="ties")
    assert got.pred.tolist() == [[[7, 2], [5, 4], [0, 0]], [[0, 0], [10, 8], [0, 0]]]
    assert got.valid.tolist() == [2, 2, 2] and got.hits.tolist() == [0, 1, 0]
    # the same maxima twice in the TARGET: its first index decides whether the joint counts
    t2 = np.zeros((1, 1, h, w), np.float32)
    t2[0, 0, 1, 6] = t2[0, 0, 5, 6] = 1.0                      # first maximum at y = 1: ignored
    got, _ = check_tensor(out[:1, :1], t2, np.ones((1, 1), np.float32), what="target tie")
    assert got.valid.tolist() == [0] and got.acc.tolist() == [0.0, -1.0] and got.cnt == 0


def test_target_peak_at_one_is_ignored_at_two_is_counted():
    h, w = 12, 10
    mu = np.array([[[1.0, 5.0], [5.0, 1.0], [2.0, 5.0], [5.0, 2.0], [1.2, 1.3], [2.0, 2.0]]])   # [1, 6, 2]
    vis = np.ones((1, 6), np.float32)
    target, tw = _val_ref.joint_targets(mu, vis, h, w)
    out = target + np.float32(0.01)
    got, _ = check_tensor(out, target, tw, what="peak at 1 / 2")
    assert got.valid.tolist() == [0, 0, 1, 1, 0, 1] and got.hits.tolist() == [0, 0, 1, 1, 0, 1]
    assert got.acc.tolist() == [1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0] and got.cnt == 3
    got, _ = check_analytic(out, mu, vis, what="peak at 1 / 2, analytic")
    assert got.valid.tolist() == [0, 0, 1, 1, 0, 1]


def test_dist_of_exactly_one_half_is_not_a_hit():
    """h = w = 20: norm = 2, a 1-px offset gives dist = 0.5 exactly, and the comparison is `<`"""
    h = w = 20
    mu = np.array([[[10.0, 9.0], [10.0, 9.0], [10.0, 9.0]]])
    vis = np.ones((1, 3), np.float32)
    target, tw = _val_ref.joint_targets(mu, vis, h, w)
    out = _blank(1, 3, h, w)
    out[0, 0, 9, 10] = 1.0       # offset 0
    out[0, 1, 9, 11] = 1.0       # 1 px in x
    out[0, 2, 10, 10] = 1.0      # 1 px in y
    got, _ = check_tensor(out, target, tw, what="dist 0.5")
    assert got.acc.tolist() == [1.0 / 3.0, 1.0, 0.0, 0.0] and got.hits.tolist() == [1, 0, 0] and got.valid.tolist() == [1, 1, 1]
    got, _ = check_analytic(out, mu, vis, what="dist 0.5, analytic")
    assert got.hits.tolist() == [1, 0, 0]


def test_invisible_joints():
    rng = np.random.default_rng(3)
    S, J, h, w = 4, 5, 17, 13                        # odd h * w: map bases only 4-byte aligned
    mu = np.stack([rng.uniform(3, w - 3, (S, J)), rng.uniform(3, h - 3, (S, J))], 2)
    mu = np.floor(mu) + 0.25
    vis = np.ones((S, J), np.float32)
    vis[:, 2] = 0                                    # joint 2 invisible in every crop: acc -1, out of cnt
    vis[1, 0] = 0.5                                  # not drawn, yet weighted in the loss
    target, tw = _val_ref.joint_targets(mu, vis, h, w)
    out = (target + rng.normal(0, 0.02, target.shape)).astype(np.float32)
    jw = np.asarray(caller.JOINTS_WEIGHT["crowdpose"][:J], np.float32) * np.float32(1.1)
    for use_w in (1, 0):
        got, _ = check_analytic(out, mu, vis, use_w=use_w, jw=jw, what="invisible joint, use_w %d" % use_w)
        assert got.acc[3] == -1.0 and got.cnt == J - 1 and got.valid.tolist() == [S - 1, S, 0, S, S]
    target_w, tw_w = _val_ref.joint_targets(mu, vis, h, w, joints_weight=jw)
    check_tensor(out, target_w, tw_w, what="invisible joint, tensor")
    none = np.zeros((S, J), np.float32)              # all joints invisible: avg_acc 0, cnt 0, acc[0] 0
    got, _ = check_analytic(out, mu, none, what="all invisible")
    assert got.cnt == 0 and got.avg_acc == 0.0 and got.acc.tolist() == [0.0] + [-1.0] * J and got.valid.tolist() == [0] * J
    assert got.loss == 0.0                           # every weight is 0: every term is (p * 0 - 0 * 0)^2
    got, _ = check_analytic(out, mu, none, use_w=False, what="all invisible, unweighted")
    assert got.cnt == 0 and got.loss > 0


@pytest.mark.parametrize("shape", [(1, 1, 7, 5), (1, 1, 1, 1), (2, 17, 96, 72), (3, 2, 20, 20), (70, 33, 8, 6)])
def test_shapes_and_alignments(shape):
    """one map, one pixel, the 96 x 72 maps of the 288-px configs, more crops than a wave has lanes and more joints than the finishing
    workgroup has waves; every shape also with the maps shifted off their 16-byte boundary (the scalar path)"""
    S, J, h, w = shape
    rng = np.random.default_rng([S, J, h, w])
    mu = np.stack([rng.uniform(-4, w + 4, (S, J)), rng.uniform(-4, h + 4, (S, J))], 2)
    mu = np.floor(mu) + rng.choice([0.125, 0.25, 0.75], (S, J, 2))
    vis = (rng.random((S, J)) > 0.2).astype(np.float32)
    target, tw = _val_ref.joint_targets(mu, vis, h, w)
    out = np.round((target + rng.normal(0, 0.05, target.shape)) * 4096) / 4096
    out = out.astype(np.float32)
    if S > 1:
        out[-1] = np.roll(out[-1], (2, 2), (1, 2))
    for off in (0, 1):
        check_tensor(out, target, tw, what="%s tensor off %d" % (shape, off), out_offset=off)
        check_analytic(out, mu, vis, what="%s analytic off %d" % (shape, off), out_offset=off)
    tw_d, t_d = run_targets(mu, vis, h, w)
    assert np.array_equal(tw_d.get().reshape(S, J), tw) and np.abs(t_d.get().reshape(target.shape).astype(np.float64) - target).max() <= DELTA


def test_two_runs_are_bit_identical():
    d = case(4)
    for kw in (dict(target=d.target, target_weight=d.target_weight), dict(joints_hm=d.joints_hm, joints_vis=d.joints_vis)):
        a, _ = run_metrics(d.output, **kw)
        b, _ = run_metrics(d.output, **kw)
        for n in ("sse", "acc", "hits", "valid", "pred"):
            assert np.array_equal(getattr(a, n), getattr(b, n)), n
        assert np.float64(a.loss).view(np.uint64) == np.float64(b.loss).view(np.uint64) and a.avg_acc == b.avg_acc and a.cnt == b.cnt


def test_no_crops_and_bad_arguments_are_codes_not_launches():
    d = case(1)
    ok = dict(target=d.target, target_weight=d.target_weight)
    z = np.zeros((0, d.J, d.h, d.w), np.float32)
    meter = torch.full((4 + 2 * GUARD,), CANARY[torch.float64], dtype=torch.float64, device=dev())
    _, o = run_metrics(z, target=z, target_weight=np.zeros((0, d.J), np.float32), meter=meter.data_ptr() + 8 * GUARD)
    assert o.untouched() and (meter == CANARY[torch.float64]).all(), "S == 0: I2R_OK, nothing launched, the meter untouched"
    _, o = run_metrics(z, joints_hm=np.zeros((0, d.J, 2)), joints_vis=np.zeros((0, d.J), np.float32))
    assert o.untouched()
    for bad in (dict(joints=0), dict(h=0), dict(w=0), dict(joints=-1), dict(n_crops=-1)):
        _, o = run_metrics(d.output, expect=-1, **ok, **bad)
        assert o.untouched(), bad
    _, o = run_metrics(d.output, expect=-1)                                       # neither target form
    assert o.untouched() and b"target form" in cabi.lib().i2r_last_error()
    _, o = run_metrics(d.output, joints_hm=d.joints_hm, joints_vis=d.joints_vis, expect=-1, **ok)   # both
    assert o.untouched()
    _, o = run_metrics(d.output, joints_hm=d.joints_hm, expect=-1)                # analytic without joints_vis
    assert o.untouched()
    _, o = run_metrics(d.output, target=d.target, expect=-1)                      # weighted loss without weights
    assert o.untouched()
    _, o = run_metrics(d.output, expect=-1, sse=None, **ok)                       # a result pointer missing
    assert o.untouched()
    tw, t = run_targets(d.joints_hm[:0], d.joints_vis[:0], d.h, d.w)
    assert tw.untouched() and t.untouched()
    for bad in (dict(joints=0), dict(h=0), dict(w=-2), dict(sigma=0.0), dict(n_crops=-1)):
        tw, t = run_targets(d.joints_hm, d.joints_vis, d.h, d.w, expect=-1, kw=bad)
        assert tw.untouched() and t.untouched(), bad
    # the Python surface: a batch without crops gives zeros and leaves the meter alone
    vm = caller.ValMeter(dev())
    m = caller.val_metrics(torch.zeros(0, d.J, d.h, d.w, device=dev()), joints_hm=np.zeros((0, d.J, 2)), joints_vis=np.zeros((0, d.J)), meter=vm)
    assert m.loss.item() == 0 and m.acc.tolist() == [0.0] * (d.J + 1) and m.cnt.item() == 0 and m.pred.shape == (0, d.J, 2)
    assert vm.buf.tolist() == [0.0] * 4 and vm.result() == (0.0, 0.0)
    with pytest.raises(cabi.I2RError):
        caller.val_metrics(torch.zeros(1, 1, 4, 4, device=dev()))


def test_meter_is_the_two_average_meters(monkeypatch):
    """three batches of different S through ValMeter = AverageMeter.update(loss, S) / .update(avg_acc, cnt) on the per-batch results;
    nothing is copied to the host before result()"""
    d = case(2)
    meter = caller.ValMeter(dev())
    per = []
    out_dev = up(d.output, np.float32)
    hm, vis = up(d.joints_hm, np.float64), up(d.joints_vis, np.float32)
    syncs = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    for sl in (slice(0, 5), slice(1, 3), slice(4, 5)):
        per.append(caller.val_metrics(out_dev[sl], joints_hm=hm[sl], joints_vis=vis[sl], joints_weight=d.jw.copy(), meter=meter))
    assert syncs == [], "val_metrics runs without a host synchronisation"
    got = meter.result()
    assert syncs == ["cpu"], "result() is the one copy to the host"
    monkeypatch.undo()
    ls = ln = as_ = an = 0.0
    for m, n in zip(per, (5, 2, 1)):
        ls, ln = ls + m.loss.item() * n, ln + n
        as_, an = as_ + m.avg_acc.item() * m.cnt.item(), an + m.cnt.item()
    assert got[0] == pytest.approx(ls / ln, rel=1e-12, abs=0) and got[1] == pytest.approx(as_ / an, rel=1e-12, abs=0)
    assert len({m.loss.item() for m in per}) == 3
    meter.reset()
    assert meter.buf.tolist() == [0.0] * 4


def test_end_to_end_forward_flip_val_metrics():
    """tph_l21 through forward_flip -> val_metrics in analytic mode; the joints sit at the arg-max of the golden heat maps plus a fixed
    offset table, so hits, misses and cut-off joints all occur; against the restatement on the same device heat maps copied to the host"""
    cfg, sd, x, m, length, g = setup("tph_l21")
    net = models.interformer.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    y = net.forward_flip(x.cuda(), m.cuda(), length, caller.FLIP_PAIRS["crowdpose"])
    S, J, h, w = y.shape
    assert (w, h) == tuple(cfg.MODEL.HEATMAP_SIZE) and J == cfg.MODEL.NUM_JOINTS == 14
    peak = _val_ref.max_preds(g["out_multi"]).astype(np.float64)                       # [S, J, 2]
    offsets = np.array([[0.25, -0.25], [0.0, 0.3], [1.25, 0.0], [-0.3, 2.2], [4.25, 3.75], [-60.0, 0.25], [0.3, 80.0]])
    mu = peak + offsets[(np.arange(S)[:, None] * 3 + np.arange(J)[None, :]) % len(offsets)]
    vis = np.ones((S, J), np.float32)
    vis[0, 3] = vis[2, 5] = 0
    meter = caller.ValMeter(y.device)
    got = caller.val_metrics_cfg(cfg, y, joints_hm=mu, joints_vis=vis, meter=meter)
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    target, tw = _val_ref.joint_targets(mu, vis, h, w, cfg.MODEL.SIGMA)
    want = _val_ref.val_metrics(out, target, tw, cfg.LOSS.USE_TARGET_WEIGHT)
    r = _val_ref.Result()
    r.loss, r.avg_acc, r.cnt = got.loss.item(), got.avg_acc.item(), got.cnt.item()
    r.acc, r.pred, r.hits, r.valid = got.acc.cpu().numpy(), got.pred.cpu().numpy(), got.hits.cpu().numpy(), got.valid.cpu().numpy()
    assert_discrete_equal(r, want, "end to end")
    assert 0 < want.valid.sum() < S * J and (tw == 0).any()
    bound = analytic_loss_bound(out, target, tw, cfg.LOSS.USE_TARGET_WEIGHT)
    print("end to end: loss %.17g, restated %.17g, |diff| %.3g, bound %.3g" % (r.loss, want.loss, abs(r.loss - want.loss), bound))
    assert abs(r.loss - want.loss) <= bound
    assert meter.result() == (pytest.approx(r.loss, rel=1e-12), pytest.approx(r.avg_acc, rel=1e-12))
    assert np.array_equal(got.pred.cpu().numpy(), _val_ref.max_preds(out))
