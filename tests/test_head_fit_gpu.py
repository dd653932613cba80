"""-m gpu: i2r_head_grad (the gradient of the validation loss with respect to final_layer, on frozen features) through the raw C-ABI on
NaN-filled workspace and outputs, against the float64 reference and the derived bound of tests/_head_fit_ref.py; exact integer cases;
edges; determinism; argument codes; consistency with i2r_val_metrics; and end to end behind a model: head_input, HeadFit, commit."""
import ctypes

import numpy as np
import pytest
import torch

import _head_fit_ref as ref
import _val_ref
from _golden import setup
from i2r_amd import cabi, caller, config, models
from test_val_metrics import CASES, case
from test_val_metrics_gpu import SUM_RTOL, analytic_loss_bound

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev():
    return torch.device("cuda", 0)


def up(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(dev())


def ws_bytes(S, h, w, cin, J):
    n = ctypes.c_int64(-1)
    assert cabi.lib().i2r_head_grad_ws_bytes(S, h, w, cin, J, ctypes.byref(n)) == 0
    return n.value


def run_grad(feat, w, b, cin, target=None, tw=None, mu=None, vis=None, jw=None, sigma=2, use_w=True, expect=0, poison=NAN, feat_offset=0, **kw):
    """the raw C-ABI call.  feat [S, h, w, cs], w [J, w_cs] numpy (channels / columns [0, cin) are read); workspace and outputs are filled
    with `poison` first.  -> namespace dw [J, cin], db, loss, sse, poisoned (True: every output still holds its poison)"""
    S, h, wd, cs = feat.shape
    J = w.shape[0]
    keep = {}
    ft = torch.zeros(feat.size + 4 + feat_offset, dtype=torch.float32, device=dev())     # (+ 4: a zero-crop tensor still has an address)
    ft[feat_offset:feat_offset + feat.size] = up(feat, np.float32).reshape(-1)
    nws = max(ws_bytes(S, h, wd, cin, J) if expect == 0 else 1 << 20, 8)
    ws = torch.full((nws // 8 + 1,), poison, dtype=torch.float64, device=dev())
    dw = torch.full((J * cin + 1,), poison, dtype=torch.float32, device=dev())            # (+ 1: a canary behind the dense rows)
    db = torch.full((J + 1,), poison, dtype=torch.float32, device=dev())
    f64 = torch.full((1 + J + 1,), poison, dtype=torch.float64, device=dev())
    keep["w"], keep["b"] = up(w, np.float32), up(b, np.float32)
    a = cabi.HeadGradArgs(feat=ft.data_ptr() + 4 * feat_offset, w=keep["w"].data_ptr(), bias=keep["b"].data_ptr(), ws=ws.data_ptr(),
                          dw=dw.data_ptr(), db=db.data_ptr(), loss=f64.data_ptr(), sse=f64.data_ptr() + 8, sigma=float(sigma), n_crops=S, h=h, w_=wd,
                          cin=cin, in_cs=cs, w_cs=w.shape[1], joints=J, use_target_weight=int(bool(use_w)))
    for name, v, dt in (("target", target, np.float32), ("target_weight", tw, np.float32), ("joints_hm", mu, np.float64),
                        ("joints_vis", vis, np.float32), ("joints_weight", jw, np.float32)):
        if v is not None:
            keep[name] = up(v, dt)
            setattr(a, name, keep[name].data_ptr() if keep[name].numel() else 16)
    for k, v in kw.items():
        setattr(a, k, v)
    rc = cabi.lib().i2r_head_grad(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    r = ref.types.SimpleNamespace()
    r.dw, r.db = dw.cpu().numpy()[:-1].reshape(J, cin), db.cpu().numpy()[:-1]
    out = f64.cpu().numpy()
    r.loss, r.sse = float(out[0]), out[1:-1]
    same = (lambda t: bool(torch.isnan(t).all())) if poison != poison else (lambda t: bool((t == poison).all()))
    r.poisoned = same(dw) and same(db) and same(f64)
    assert same(dw[-1:]) and same(db[-1:]) and same(f64[-1:]), "canary behind an output overwritten"
    return r


def multi(y):
    return y["multi"] if isinstance(y, dict) else y


def check(got, want, what, names=("dw", "db", "loss", "sse")):
    """every output within its bound of the float64 reference; prints got, wanted, |diff| and bound at the worst element"""
    for name in names:
        bound = getattr(want, "b_" + name)
        g, w_, bd = (np.asarray(v, np.float64).reshape(-1) for v in (getattr(got, name), getattr(want, name), bound))
        diff = np.abs(g - w_)
        i = int(np.argmax(diff - bd))
        print("%s %s: got %.9g wanted %.9g |diff| %.3g bound %.3g (max |diff| / bound %.3g)"
              % (what, name, g[i], w_[i], diff[i], bd[i], float(np.max(diff / np.where(bd > 0, bd, 1e-300)))))
        assert np.isfinite(g).all() and (diff <= bd).all(), (what, name, g[i], w_[i], diff[i], bd[i])


def head_problem(ci, cin, seed=0):
    """the fixture's joints of case ci with random features / weights: in_cs > cin and w_cs > cin, NaN in the channels that must not be
    read, a joints_weight table at every case, cin 80 with 78 non-zero channels"""
    d = case(ci)
    rng = np.random.default_rng([seed, ci, cin])
    p = ref.types.SimpleNamespace(S=d.S, J=d.J, h=d.h, w_=d.w, cin=cin)
    p.feat = rng.standard_normal((d.S, d.h, d.w, cin + 4)).astype(np.float32)
    p.w = (rng.standard_normal((d.J, cin + 3)) * 0.3 / np.sqrt(cin)).astype(np.float32)
    if cin == 80:
        p.feat[..., 78:] = 0
        p.w[:, 78:] = 0
    p.feat[..., cin:] = NAN
    p.w[:, cin:] = NAN
    p.b = (rng.standard_normal(d.J) * 0.1).astype(np.float32)
    p.mu, p.vis = d.joints_hm, d.joints_vis
    p.jw = d.jw if d.jw is not None else (1.0 + 0.1 * (np.arange(d.J) % 4)).astype(np.float32)
    p.target, p.tw = _val_ref.joint_targets(p.mu, p.vis, d.h, d.w, d.sigma, p.jw)
    p.drawn = _val_ref.joint_targets(p.mu, p.vis, d.h, d.w, d.sigma, None)[1] > 0.5
    return p


def test_the_fixture_holds_undrawn_weighted_and_cut_off_joints():
    undrawn = cut = 0
    for ci in range(len(CASES)):
        p, d = head_problem(ci, 16), case(ci)
        undrawn += int(((p.vis == 0.5) & (p.tw > 0) & ~p.drawn).sum())
        cut += int(((p.vis == 1) & (p.tw == 0)).sum())
        if d.S * d.J > 1:
            assert all(p.tw[s, j] == 0 and d.joints_vis[s, j] == 1 for k, (s, j) in enumerate(d.plants) if k % 2 == 0)
    assert undrawn > 0 and cut > 0


@pytest.mark.parametrize("cin", [16, 80, 128])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_both_forms_meet_the_bound(ci, cin):
    p = head_problem(ci, cin)
    for use_w in (True, False):
        want_t = ref.head_grad64(p.feat, p.w[:, :cin], p.b, p.target, p.tw, use_w)
        got = run_grad(p.feat, p.w, p.b, cin, target=p.target, tw=p.tw, use_w=use_w)
        check(got, want_t, "case %d cin %d use_w %d tensor" % (ci, cin, use_w))
        want_a = ref.head_grad64(p.feat, p.w[:, :cin], p.b, p.target, p.tw, use_w, drawn=p.drawn)
        got = run_grad(p.feat, p.w, p.b, cin, mu=p.mu, vis=p.vis, jw=p.jw, use_w=use_w)
        check(got, want_a, "case %d cin %d use_w %d analytic" % (ci, cin, use_w))
    got = run_grad(p.feat, p.w, p.b, cin, target=p.target, use_w=False)     # no weights at all
    check(got, want_t, "case %d cin %d unweighted, null target_weight" % (ci, cin))


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 4, 8, 8, 16), (3, 17, 7, 5, 32), (1, 32, 16, 8, 16)])
def test_integer_problems_are_exact(shape):
    """small integers: every partial sum stays below 2^24, so fp32 and float64 agree exactly.  N J a power of two: dw N J, db N J are the
    integers themselves; otherwise dw is the ONE rounding of integer / (N J)"""
    S, J, h, w, cin = shape
    rng = np.random.default_rng(shape)
    feat, wt, b, t = _ints(rng, -2, 2, (S, h, w, cin)), _ints(rng, -2, 2, (J, cin)), _ints(rng, -3, 3, (J,)), _ints(rng, -4, 4, (S, J, h, w))
    NJ = S * h * w * J
    F = feat.astype(np.int64).reshape(S, h * w, cin)
    o = np.einsum("spc,jc->sjp", F, wt.astype(np.int64)) + b.astype(np.int64)[None, :, None]
    g = o - t.astype(np.int64).reshape(S, J, -1)
    gi, bi, si = np.einsum("sjp,spc->jc", g, F), g.sum((0, 2)), (g * g).sum((0, 2))
    assert np.abs(gi).max() < 2 ** 24 and si.max() < 2 ** 53
    got = run_grad(feat, wt, b, cin, target=t, use_w=False)
    assert np.array_equal(got.sse, si.astype(np.float64)) and got.loss == float((0.5 * (si / (S * h * w))).sum() / J)
    assert np.array_equal(got.dw, (gi / NJ).astype(np.float32)) and np.array_equal(got.db, (bi / NJ).astype(np.float32))
    if NJ & (NJ - 1) == 0:
        assert np.array_equal(got.dw.astype(np.float64) * NJ, gi) and np.array_equal(got.db.astype(np.float64) * NJ, bi)
    # analytic form, every visibility 0.5: nothing is drawn (t = 0), tw = 0.5, tw^2 = 0.25
    mu = np.stack([rng.uniform(2, w - 2, (S, J)), rng.uniform(2, h - 2, (S, J))], 2)
    got = run_grad(feat, wt, b, cin, mu=mu, vis=np.full((S, J), 0.5, np.float32), use_w=True)
    go = np.einsum("sjp,spc->jc", o, F)
    assert np.array_equal(got.sse, 0.25 * (o * o).sum((0, 2)))
    assert np.array_equal(got.dw, (0.25 * go / NJ).astype(np.float32)) and np.array_equal(got.db, (0.25 * o.sum((0, 2)) / NJ).astype(np.float32))
    if NJ & (NJ - 1) == 0:
        assert np.array_equal(got.dw.astype(np.float64) * NJ, 0.25 * go)


@pytest.mark.parametrize("J", [1, 16, 17, 32])
@pytest.mark.parametrize("hw", [(7, 5), (17, 13)])
def test_edges(hw, J):
    """h w of 35 and 221 (no multiple of a fragment), one crop and three, joint counts around the 16-wide fragments; one pixel with
    features 50 times the rest; a crop whose joints are all invisible"""
    h, w = hw
    for S in (1, 3):
        p = ref.problem(S, J, h, w, 32, seed=5, cs=36)
        p.feat[S - 1, h - 1, w - 1, :32] *= 50
        for use_w in (True, False):
            want = ref.head_grad64(p.feat, p.w, p.b, p.target, p.tw, use_w, drawn=p.drawn)
            check(run_grad(p.feat, p.w, p.b, 32, mu=p.mu, vis=p.vis, jw=p.jw, use_w=use_w), want, "%dx%d J %d S %d use_w %d analytic" % (h, w, J, S, use_w))
            want = ref.head_grad64(p.feat, p.w, p.b, p.target, p.tw, use_w)
            check(run_grad(p.feat, p.w, p.b, 32, target=p.target, tw=p.tw, use_w=use_w), want, "%dx%d J %d S %d use_w %d tensor" % (h, w, J, S, use_w))
    # the last crop invisible: it adds nothing, so the sums are those of the first two crops (N differs: an exact factor in fp32)
    vis = p.vis.copy()
    vis[2] = 0
    a = run_grad(p.feat, p.w, p.b, 32, mu=p.mu, vis=vis, jw=p.jw)
    b = run_grad(p.feat[:2], p.w, p.b, 32, mu=p.mu[:2], vis=vis[:2], jw=p.jw)
    assert not b.poisoned
    want = ref.head_grad64(p.feat[:2], p.w, p.b, p.target[:2], p.tw[:2], True, drawn=p.drawn[:2])
    scaled = ref.types.SimpleNamespace(dw=a.dw.astype(np.float64) * 1.5, db=a.db.astype(np.float64) * 1.5, loss=a.loss * 1.5, sse=a.sse)
    check(scaled, want, "%dx%d J %d invisible crop" % (h, w, J))


def test_two_runs_and_another_poison_give_the_same_bits():
    p = head_problem(4, 128)
    for kw in (dict(target=p.target, tw=p.tw), dict(mu=p.mu, vis=p.vis, jw=p.jw)):
        a = run_grad(p.feat, p.w, p.b, 128, **kw)
        b = run_grad(p.feat, p.w, p.b, 128, **kw)
        c = run_grad(p.feat, p.w, p.b, 128, poison=-3.0e30, **kw)
        for o in (b, c):
            assert np.array_equal(a.dw.view(np.uint32), o.dw.view(np.uint32)) and np.array_equal(a.db.view(np.uint32), o.db.view(np.uint32))
            assert np.array_equal(a.sse.view(np.uint64), o.sse.view(np.uint64)) and np.float64(a.loss).view(np.uint64) == np.float64(o.loss).view(np.uint64)


def test_no_crops_and_bad_arguments_are_codes_not_launches():
    p = head_problem(1, 16)
    ok = dict(target=p.target, tw=p.tw)
    z = np.zeros((0, p.h, p.w_, 20), np.float32)
    r = run_grad(z, p.w, p.b, 16, target=np.zeros((0, p.J, p.h, p.w_), np.float32), tw=np.zeros((0, p.J), np.float32))
    assert r.poisoned, "n_crops == 0: I2R_OK, nothing launched, nothing written"
    assert run_grad(z, p.w, p.b, 16, mu=np.zeros((0, p.J, 2)), vis=np.zeros((0, p.J), np.float32)).poisoned
    w33 = np.zeros((33, 19), np.float32)
    assert run_grad(p.feat, w33, np.zeros(33, np.float32), 16, target=np.zeros((p.S, 33, p.h, p.w_), np.float32), use_w=False, expect=-1).poisoned
    big = np.zeros((p.S, p.h, p.w_, 148), np.float32)
    wbig = np.zeros((p.J, 148), np.float32)
    for cin in (24, 144, 0):
        assert run_grad(big, wbig, p.b, cin, expect=-1, **ok).poisoned, cin
    assert run_grad(p.feat, p.w, p.b, 16, mu=p.mu, vis=p.vis, expect=-1, **ok).poisoned, "both target forms"
    r = run_grad(p.feat, p.w, p.b, 16, expect=-1)
    assert r.poisoned and b"target form" in cabi.lib().i2r_last_error(), "neither target form"
    assert run_grad(p.feat, p.w, p.b, 16, feat_offset=1, expect=-1, **ok).poisoned, "feat off its 16-byte boundary"
    assert run_grad(p.feat, p.w, p.b, 16, target=p.target, expect=-1).poisoned, "a weighted loss without weights"
    assert run_grad(p.feat, p.w, p.b, 16, mu=p.mu, expect=-1).poisoned, "the analytic form without joints_vis"
    for bad in (dict(in_cs=12), dict(in_cs=18), dict(w_cs=12), dict(h=0), dict(n_crops=-1), dict(joints=0), dict(dw=None), dict(ws=None)):
        assert run_grad(p.feat, p.w, p.b, 16, expect=-1, **ok, **bad).poisoned, bad
    assert run_grad(p.feat, p.w, p.b, 16, mu=p.mu, vis=p.vis, sigma=0.0, expect=-1).poisoned
    # the Python surface
    ft = torch.zeros(0, p.h, p.w_, 16, device=dev())
    g = caller.head_grad(ft, torch.zeros(p.J, 16, 1, 1), torch.zeros(p.J), joints_hm=np.zeros((0, p.J, 2)), joints_vis=np.zeros((0, p.J)))
    assert g.loss.item() == 0 and g.dw.shape == (p.J, 16) and not g.dw.any() and not g.db.any()
    with pytest.raises(cabi.I2RError):
        caller.head_grad(torch.zeros(1, 4, 4, 16, device=dev()), torch.zeros(2, 16), torch.zeros(2))


@pytest.mark.parametrize("ci", [1, 3])
def test_loss_agrees_with_val_metrics_on_the_applied_head(ci):
    """caller.head_grad against caller.val_metrics on caller.head_apply's heat maps, both target forms; without a host synchronisation"""
    p = head_problem(ci, 80)
    feat = up(np.nan_to_num(p.feat), np.float32)
    wt, b = up(p.w[:, :78], np.float32), up(p.b, np.float32)          # a 78-channel head: padded to 80 inside
    out = caller.head_apply(feat, wt, b)
    assert out.shape == (p.S, p.J, p.h, p.w_)
    want = ref.head_grad64(p.feat, p.w[:, :80], p.b, p.target, p.tw, True, drawn=p.drawn)
    assert (np.abs(out.cpu().numpy().astype(np.float64).reshape(p.S, p.J, -1) - want.o) <= want.e_o).all()
    for form in ("tensor", "analytic"):
        if form == "tensor":
            kw = dict(target=up(p.target, np.float32), target_weight=up(p.tw, np.float32))
            vm = caller.val_metrics(out, kw["target"], kw["target_weight"])
            g = caller.head_grad(feat, wt, b, kw["target"], kw["target_weight"])
            vm_bound = SUM_RTOL * vm.loss.item()
            w64 = ref.head_grad64(p.feat, p.w[:, :80], p.b, p.target, p.tw, True)
        else:
            kw = dict(joints_hm=p.mu.copy(), joints_vis=p.vis.copy(), joints_weight=p.jw.copy())
            vm = caller.val_metrics(out, **kw)
            g = caller.head_grad(feat, wt, b, **kw)
            vm_bound = analytic_loss_bound(out.cpu().numpy(), p.target, p.tw, True)
            w64 = want
        diff = abs(g.loss.item() - vm.loss.item())
        print("case %d %s: head_grad loss %.17g, val_metrics %.17g, |diff| %.3g, bound %.3g + %.3g" % (ci, form, g.loss.item(), vm.loss.item(), diff, w64.b_loss, vm_bound))
        assert diff <= w64.b_loss + vm_bound
        assert g.dw.shape == (p.J, 78)
        got = ref.types.SimpleNamespace(dw=g.dw.cpu().numpy(), db=g.db.cpu().numpy(), loss=g.loss.item(), sse=g.sse.cpu().numpy())
        w64.dw, w64.b_dw = w64.dw[:, :78], w64.b_dw[:, :78]
        check(got, w64, "case %d %s through caller.head_grad" % (ci, form))


def test_head_grad_runs_without_a_host_synchronisation(monkeypatch):
    p = head_problem(2, 16)
    feat, wt, b = up(np.nan_to_num(p.feat), np.float32), up(p.w[:, :16], np.float32), up(p.b, np.float32)
    hm, vis = up(p.mu, np.float64), up(p.vis, np.float32)
    fit = caller.HeadFit(16, p.J, wt, b)
    syncs = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    caller.head_grad(feat, wt, b, joints_hm=hm, joints_vis=vis)
    caller.head_apply(feat, wt, b)
    fit.grad(feat, joints_hm=hm, joints_vis=vis)
    assert syncs == []


# ---- end to end behind a model --------------------------------------------------------------------------------------------------------

_E2E = {}


def e2e():
    if not _E2E:
        cfg, sd, x, m, length, g = setup("tph_l21")
        net = models.interformer.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        net = net.cuda()
        x, m = x.cuda(), m.cuda()
        hi = net.head_input(x, m, length)
        y = multi(net(x, m, length))
        torch.cuda.synchronize()
        _E2E.update(cfg=cfg, sd=sd, x=x, m=m, length=length, net=net, hi=hi, y=y, g=g)
    return ref.types.SimpleNamespace(**_E2E)


def _targets(e):
    """joints at the arg-max of the golden heat maps plus a fixed offset table (hits, misses, cut-off joints), two invisible, one at 0.5"""
    S, J, h, w = e.y.shape
    peak = _val_ref.max_preds(e.g["out_multi"]).astype(np.float64)
    offsets = np.array([[0.25, -0.25], [0.0, 0.3], [1.25, 0.0], [-0.3, 2.2], [4.25, 3.75], [-60.0, 0.25], [0.3, 80.0]])
    mu = peak + offsets[(np.arange(S)[:, None] * 3 + np.arange(J)[None, :]) % len(offsets)]
    vis = np.ones((S, J), np.float32)
    vis[0, 3] = vis[2, 5] = 0
    vis[1, 0] = 0.5
    return mu, vis


def test_head_input_is_the_forward_and_the_tensor_the_head_reads():
    e = e2e()
    S, J, h, w = e.y.shape
    assert torch.equal(e.hi.heatmaps, e.y), "head_input's heat maps are the forward's, bit for bit"
    feat, cin = e.hi.feat, e.hi.cin
    assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.shape[:3] == (S, h, w) and feat.shape[3] >= cin
    assert cin == e.sd["final_layer.weight"].shape[1] and not feat[..., cin:].any()
    again = e.net.head_input(e.x, e.m, e.length)
    assert again.feat.data_ptr() != feat.data_ptr() and torch.equal(again.feat, feat), "a copy per call: the next forward overwrites the arena"
    wt, b = e.sd["final_layer.weight"].reshape(J, cin).numpy(), e.sd["final_layer.bias"].numpy()
    r = ref.head_grad64(feat.cpu().numpy(), wt, b, np.zeros((S, J, h, w)), np.ones((S, J)), False)
    diff = np.abs(e.y.cpu().numpy().astype(np.float64).reshape(S, J, -1) - r.o)
    print("W feat + b in float64 against the forward's heat maps: max |diff| %.3g, max |diff| / e_o %.3g" % (diff.max(), (diff / r.e_o).max()))
    assert (diff <= r.e_o).all()
    assert torch.equal(caller.head_apply(feat, e.sd["final_layer.weight"].cuda(), e.sd["final_layer.bias"].cuda()), e.y)


def test_head_input_refusals():
    for tag, fn in (("w48_fk3_l21", models.interformer_pureMulti), ("tph_win_l12", models.interformer)):
        cfg, sd, x, m, length, _ = setup(tag)
        net = fn.get_pose_net(cfg, is_train=False)
        net.load_state_dict(sd, strict=True)
        with pytest.raises(ValueError):
            net.cuda().head_input(x.cuda(), m.cuda(), length)


def test_the_models_own_heat_maps_as_target_give_a_zero_gradient():
    e = e2e()
    S, J, h, w = e.y.shape
    fit = caller.HeadFit.from_model(e.net)
    assert isinstance(fit.optimizer, torch.optim.Adam) and fit.optimizer.defaults["lr"] == e.cfg.TRAIN.LR
    tw = torch.ones(S, J, device=e.y.device)
    g = fit.grad(e.hi.feat, e.y, tw)
    wt, b = e.sd["final_layer.weight"].reshape(J, -1).numpy(), e.sd["final_layer.bias"].numpy()
    r = ref.head_grad64(e.hi.feat.cpu().numpy(), wt, b, e.y.cpu().numpy(), np.ones((S, J)), True)
    dw, loss = g.dw.cpu().numpy(), g.loss.item()
    print("own heat maps as target: max |dw| %.3g (max |dw| / B_dw %.3g), loss %.3g (bound %.3g)" % (np.abs(dw).max(), (np.abs(dw) / r.b_dw).max(), loss, r.b_loss))
    assert (np.abs(dw - r.dw) <= r.b_dw).all() and abs(loss - r.loss) <= r.b_loss
    assert (np.abs(dw) <= r.b_dw).all() and loss <= r.b_loss            # against the exact zero


def test_gradient_descent_at_one_over_l_lowers_the_loss_every_step():
    e = e2e()
    S, J, h, w = e.y.shape
    cin, N = e.hi.cin, S * h * w
    mu, vis = _targets(e)
    sigma = e.cfg.MODEL.SIGMA
    target, tw = _val_ref.joint_targets(mu, vis, h, w, sigma)
    drawn = tw > 0.5
    assert (tw == 0).any() and ((tw > 0) & ~drawn).any()
    f = e.hi.feat.cpu().numpy()
    ft = np.concatenate([f[..., :cin].astype(np.float64).reshape(S, h * w, cin), np.ones((S, h * w, 1))], 2)
    A = np.einsum("spa,spb->sab", ft, ft)
    L = max(float(np.linalg.eigvalsh(np.einsum("s,sab->ab", tw[:, j].astype(np.float64) ** 2, A) / (N * J))[-1]) for j in range(J))
    fit = caller.HeadFit(cin, J, torch.zeros(J, cin, 1, 1), torch.zeros(J), optimizer=lambda ps: torch.optim.SGD(ps, lr=1.0 / L))
    losses = []
    for step in range(10):
        wt, b = fit.weight.detach().cpu().numpy().reshape(J, cin), fit.bias.detach().cpu().numpy()
        losses.append(fit.step(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma).item())
        r = ref.head_grad64(f, wt, b, target, tw, True, drawn=drawn)
        got = ref.types.SimpleNamespace(dw=fit.weight.grad.cpu().numpy().reshape(J, cin), db=fit.bias.grad.cpu().numpy(), loss=losses[-1])
        check(got, r, "step %d (L %.4g)" % (step, L), names=("dw", "db", "loss"))
    losses.append(fit.grad(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma).loss.item())
    print("losses", ["%.6g" % v for v in losses])
    assert all(b < a for a, b in zip(losses, losses[1:]))


def test_commit_puts_the_head_into_the_model():
    e = e2e()
    S, J, h, w = e.y.shape
    cin = e.hi.cin
    net = models.interformer.get_pose_net(e.cfg, is_train=False)
    net.load_state_dict(e.sd, strict=True)
    net = net.cuda()
    rng = np.random.default_rng(8)
    wt = (rng.standard_normal((J, cin, 1, 1)) * 0.3 / np.sqrt(cin)).astype(np.float32)
    b = (rng.standard_normal(J) * 0.1).astype(np.float32)
    fit = caller.HeadFit(cin, J, torch.from_numpy(wt), torch.from_numpy(b))
    net(e.x, e.m, e.length)                      # (an engine is packed: commit has to drop it)
    fit.commit(net)
    y = multi(net(e.x, e.m, e.length))
    r = ref.head_grad64(e.hi.feat.cpu().numpy(), wt.reshape(J, cin), b, np.zeros((S, J, h, w)), np.ones((S, J)), False)
    diff = np.abs(y.cpu().numpy().astype(np.float64).reshape(S, J, -1) - r.o)
    print("after commit: max |diff| %.3g, max |diff| / e_o %.3g" % (diff.max(), (diff / r.e_o).max()))
    assert (diff <= r.e_o).all()
    st = net.state_dict()
    assert torch.equal(st["final_layer.weight"].cpu(), torch.from_numpy(wt)) and torch.equal(st["final_layer.bias"].cpu(), torch.from_numpy(b))
    assert set(fit.state()) == {"final_layer.weight", "final_layer.bias"}
    # another joint set: commit refuses; the state loads into a model built for it
    fit12 = caller.HeadFit(cin, 12)
    with pytest.raises(ValueError):
        fit12.commit(net)
    cfg12 = config.load_config("tph_192_p6_b4", ["MODEL.NUM_JOINTS", 12])
    net12 = models.interformer.get_pose_net(cfg12, is_train=False)
    have = net12.state_dict()
    state = dict({k: v for k, v in e.sd.items() if k in have and have[k].shape == v.shape}, **{k: v.cpu() for k, v in fit12.state().items()})
    net12.load_state_dict(state, strict=False)   # (a first-stage head of the old joint count keeps its fresh initialisation)
    net12 = net12.cuda()
    y12 = multi(net12(e.x, e.m, e.length))
    assert y12.shape == (S, 12, h, w) and torch.isfinite(y12).all()
    assert torch.equal(y12, caller.head_apply(net12.head_input(e.x, e.m, e.length).feat, fit12.weight, fit12.bias))
