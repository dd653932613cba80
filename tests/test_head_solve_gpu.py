"""-m gpu: i2r_head_normal (the normal equations of the head re-fit, one pass over frozen features) through the raw C-ABI on a poisoned
workspace and a state whose surroundings are poisoned, against the float64 reference and the derived bounds of tests/_head_solve_ref.py;
exact integer cases; determinism; i2r_head_grad as an independent yardstick; the solved head (caller.HeadSolve); splitting and merging;
end to end behind a model; no host synchronisation; argument codes."""
import ctypes

import numpy as np
import pytest
import torch

import _head_fit_ref as hf
import _head_solve_ref as ref
import _val_ref
from i2r_amd import cabi, caller, models
from test_head_fit_gpu import _targets, dev, e2e, multi, run_grad, up

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 3      # doubles behind cin_out + 1 in every row of the state: they, and the rows behind, must stay as they were


def ws_bytes(S, h, w, cin, J):
    n = ctypes.c_int64(-1)
    assert cabi.lib().i2r_head_normal_ws_bytes(S, h, w, cin, J, ctypes.byref(n)) == 0
    return n.value


def run_normal(feat, J, cin, target=None, tw=None, mu=None, vis=None, jw=None, sigma=2, use_w=True, expect=0, poison=NAN, state=None,
               cin_out=None, feat_offset=0, **kw):
    """the raw C-ABI call.  feat [S, h, w, cs] numpy (channels [0, cin) are read).  The workspace is filled with `poison`; the state
    (state: a namespace of an earlier call to add into, else zeros) lives in buffers with ld = cin_out + 1 + PAD whose every other
    double holds `poison`.  -> namespace A [J, m, m], r [J, m], c [J], n (numpy), touched (True: a live state element changed)"""
    S, h, wd, cs = feat.shape
    co = cin if cin_out is None else cin_out
    m, ld = co + 1, co + 1 + PAD
    keep = {}
    ft = torch.zeros(feat.size + 4 + feat_offset, dtype=torch.float32, device=dev())
    ft[feat_offset:feat_offset + feat.size] = up(feat, np.float32).reshape(-1)
    nws = max(ws_bytes(S, h, wd, cin, J) if expect == 0 else 1 << 22, 8)
    ws = torch.full((nws // 8 + 1,), poison, dtype=torch.float64, device=dev())
    A = torch.full((J * ld * ld + 1,), poison, dtype=torch.float64, device=dev())
    r = torch.full((J * ld + 1,), poison, dtype=torch.float64, device=dev())
    c = torch.full((J + 1,), poison, dtype=torch.float64, device=dev())
    n = torch.full((2,), -77, dtype=torch.int64, device=dev())
    Av, rv = A[:-1].view(J, ld, ld)[:, :m, :m], r[:-1].view(J, ld)[:, :m]
    if state is None:
        Av.zero_(), rv.zero_(), c[:J].zero_(), n[:1].zero_()
    else:
        Av.copy_(up(state.A, np.float64)), rv.copy_(up(state.r, np.float64)), c[:J].copy_(up(state.c, np.float64)), n[:1].fill_(int(state.n))
    before = [t.clone() for t in (A, r, c, n)]
    a = cabi.HeadNormalArgs(feat=ft.data_ptr() + 4 * feat_offset, ws=ws.data_ptr(), A=A.data_ptr(), r=r.data_ptr(), c=c.data_ptr(), n=n.data_ptr(),
                            sigma=float(sigma), n_crops=S, h=h, w_=wd, cin=cin, in_cs=cs, cin_out=co, ld=ld, joints=J, use_target_weight=int(bool(use_w)))
    for name, v, dt in (("target", target, np.float32), ("target_weight", tw, np.float32), ("joints_hm", mu, np.float64),
                        ("joints_vis", vis, np.float32), ("joints_weight", jw, np.float32)):
        if v is not None:
            keep[name] = up(v, dt)
            setattr(a, name, keep[name].data_ptr() if keep[name].numel() else 16)
    for k, v in kw.items():
        setattr(a, k, v)
    rc = cabi.lib().i2r_head_normal(ctypes.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect, (rc, cabi.lib().i2r_last_error())
    live = [torch.zeros_like(t, dtype=torch.bool) for t in (A, r, c, n)]
    live[0][:-1].view(J, ld, ld)[:, :m, :m] = True
    live[1][:-1].view(J, ld)[:, :m] = True
    live[2][:J] = True
    live[3][:1] = True
    q = hf.types.SimpleNamespace(touched=False)
    for t, b, lv in zip((A, r, c, n), before, live):
        same = (t == b) | ((t != t) & (b != b)) if t.dtype != torch.int64 else t == b
        assert bool(same[~lv].all()), "the state's surroundings were written"
        q.touched = q.touched or not bool(same[lv].all())
    q.A, q.r, q.c, q.n = Av.cpu().numpy().copy(), rv.cpu().numpy().copy(), c[:J].cpu().numpy().copy(), int(n[0].item())
    return q


def check(got, want, what):
    for name in ("A", "r", "c"):
        g, w_, bd = (np.asarray(v, np.float64).reshape(-1) for v in (getattr(got, name), getattr(want, name), getattr(want, "b_" + name)))
        diff = np.abs(g - w_)
        ratio = np.where(diff == 0, 0.0, diff / np.where(bd > 0, bd, 1e-300))
        i = int(np.argmax(ratio))
        print("%s %s: got %.17g wanted %.17g |diff| %.3g bound %.3g (max |diff| / bound %.3g)" % (what, name, g[i], w_[i], diff[i], bd[i], ratio[i]))
        assert np.isfinite(g).all() and (diff <= bd).all(), (what, name, g[i], w_[i], diff[i], bd[i])
    assert got.n == want.n, "n is exact"
    assert np.array_equal(got.A.view(np.uint64), np.swapaxes(got.A, 1, 2).copy().view(np.uint64)), "A is symmetric bit for bit"


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_both_forms_meet_the_bounds(shape):
    p = ref.shape_problem(shape)
    for use_w in (True, False):
        want = ref.normal64(p.feat, p.target, p.tw, p.cin, use_w)
        got = run_normal(p.feat, p.J, p.cin, target=p.target, tw=p.tw, use_w=use_w)
        check(got, want, "%s use_w %d tensor" % (shape, use_w))
        want = ref.normal64(p.feat, p.target, p.tw, p.cin, use_w, drawn=p.drawn)
        got = run_normal(p.feat, p.J, p.cin, mu=p.mu, vis=p.vis, jw=p.jw, use_w=use_w)
        check(got, want, "%s use_w %d analytic" % (shape, use_w))
    got = run_normal(p.feat, p.J, p.cin, target=p.target, use_w=False)     # no weights at all
    check(got, ref.normal64(p.feat, p.target, p.tw, p.cin, False), "%s unweighted, null target_weight" % (shape,))
    if p.cin == 80:      # a 78-channel head on the padded features: the state is that of the true cin, the bias entry at index 78
        got = run_normal(p.feat, p.J, 80, target=p.target, tw=p.tw, cin_out=78)
        check(got, ref.normal64(p.feat, p.target, p.tw, 78, True), "%s cin_out 78" % (shape,))


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 4, 8, 8, 16), (3, 17, 7, 5, 32), (1, 32, 16, 8, 128)])
def test_integer_problems_are_exact(shape):
    """small integers: every partial sum stays below 2^24, so fp32 and float64 agree exactly"""
    S, J, h, w, cin = shape
    rng = np.random.default_rng(shape)
    feat, t = _ints(rng, -2, 2, (S, h, w, cin)), _ints(rng, -4, 4, (S, J, h, w))
    Ft = np.concatenate([feat.astype(np.int64).reshape(S, h * w, cin), np.ones((S, h * w, 1), np.int64)], 2)
    G = np.einsum("spa,spb->ab", Ft, Ft)
    ti = t.astype(np.int64).reshape(S, J, -1)
    ri, ci = np.einsum("sjp,spa->ja", ti, Ft), (ti * ti).sum((0, 2))
    got = run_normal(feat, J, cin, target=t, use_w=False)
    assert np.array_equal(got.A, np.broadcast_to(G, (J,) + G.shape).astype(np.float64)) and np.array_equal(got.r, ri.astype(np.float64))
    assert np.array_equal(got.c, ci.astype(np.float64)) and got.n == S * h * w
    # weights 0, 0.5, 2 per (crop, joint): tw^2 = 0, 0.25, 4 keep everything an exact binary fraction
    tw = rng.choice([0.0, 0.5, 2.0], (S, J)).astype(np.float32)
    tw2 = tw.astype(np.float64) ** 2
    got = run_normal(feat, J, cin, target=t, tw=tw, use_w=True)
    assert np.array_equal(got.A, np.einsum("sj,sab->jab", tw2, np.einsum("spa,spb->sab", Ft, Ft).astype(np.float64)))
    assert np.array_equal(got.r, np.einsum("sj,sjp,spa->ja", tw2, ti.astype(np.float64), Ft.astype(np.float64)))
    assert np.array_equal(got.c, np.einsum("sj,sjp->j", tw2, (ti * ti).astype(np.float64)))
    # analytic form, every visibility 0.5: nothing is drawn (t = 0), tw = 0.5
    mu = np.stack([rng.uniform(2, w - 2, (S, J)), rng.uniform(2, h - 2, (S, J))], 2)
    got = run_normal(feat, J, cin, mu=mu, vis=np.full((S, J), 0.5, np.float32))
    assert np.array_equal(got.A, np.broadcast_to(0.25 * G, (J,) + G.shape)) and not got.r.any() and not got.c.any()


def test_poison_repeatability_and_adding_twice():
    p = ref.shape_problem((3, 20, 16, 12, 96))
    for kw in (dict(target=p.target, tw=p.tw), dict(mu=p.mu, vis=p.vis, jw=p.jw)):
        a = run_normal(p.feat, p.J, p.cin, **kw)
        b = run_normal(p.feat, p.J, p.cin, **kw)
        c = run_normal(p.feat, p.J, p.cin, poison=-3.0e30, **kw)
        for o in (b, c):
            assert all(np.array_equal(getattr(a, k).view(np.uint64), getattr(o, k).view(np.uint64)) for k in ("A", "r", "c")) and a.n == o.n
        twice = run_normal(p.feat, p.J, p.cin, state=a, **kw)                     # the batch again, into the state
        copied = run_normal(p.feat, p.J, p.cin, state=hf.types.SimpleNamespace(A=a.A.copy(), r=a.r.copy(), c=a.c.copy(), n=a.n), poison=5.0, **kw)
        assert all(np.array_equal(getattr(twice, k).view(np.uint64), getattr(copied, k).view(np.uint64)) for k in ("A", "r", "c"))
        assert twice.n == copied.n == 2 * a.n and np.array_equal(twice.A, 2 * a.A) and np.array_equal(twice.c, 2 * a.c)


@pytest.mark.parametrize("shape", [(3, 17, 7, 5, 32), (3, 20, 16, 12, 96)])
def test_head_grad_at_the_zero_head_is_minus_r(shape):
    """the merged gradient kernel as an independent yardstick: at W = 0, b = 0 it gives dw = -r / (n J), db likewise and sse = c"""
    p = ref.shape_problem(shape)
    J, cin = p.J, p.cin
    z, zb = np.zeros((J, cin), np.float32), np.zeros(J, np.float32)
    for form in ("tensor", "analytic"):
        kw = dict(target=p.target, tw=p.tw) if form == "tensor" else dict(mu=p.mu, vis=p.vis, jw=p.jw)
        drawn = None if form == "tensor" else p.drawn
        q = ref.normal64(p.feat, p.target, p.tw, cin, True, drawn=drawn)
        g64 = hf.head_grad64(p.feat, z, zb, p.target, p.tw, True, drawn=drawn)
        got, g = run_normal(p.feat, J, cin, **kw), run_grad(p.feat, z, zb, cin, **kw)
        nJ = q.n * J
        dw, db, sse = np.abs(g.dw + got.r[:, :cin] / nJ), np.abs(g.db + got.r[:, cin] / nJ), np.abs(g.sse - got.c)
        print("%s %s: max |dw + r / nJ| / bound %.3g, db %.3g, sse %.3g" % (shape, form, (dw / np.maximum(g64.b_dw + q.b_r[:, :cin] / nJ, 1e-300)).max(),
                                                                          (db / np.maximum(g64.b_db + q.b_r[:, cin] / nJ, 1e-300)).max(), (sse / np.maximum(g64.b_sse + q.b_c, 1e-300)).max()))
        assert (dw <= g64.b_dw + q.b_r[:, :cin] / nJ).all() and (db <= g64.b_db + q.b_r[:, cin] / nJ).all() and (sse <= g64.b_sse + q.b_c).all()


def _solver(p, cin=None, **kw):
    cin = p.cin if cin is None else cin
    acc = caller.HeadSolve(cin, p.J, device=dev())
    acc.add(up(np.nan_to_num(p.feat), np.float32), joints_hm=p.mu, joints_vis=p.vis, joints_weight=p.jw, **kw)
    return acc


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_the_solved_head_has_a_zero_gradient_and_the_least_loss(shape):
    p = ref.shape_problem(shape)
    J, cin = p.J, 78 if p.cin == 80 else p.cin
    acc = _solver(p, cin)
    assert acc.state.A.shape == (J, cin + 1, cin + 1) and acc.state.n.item() == p.S * p.h * p.w_
    w, b = acc.solve()
    assert w.shape == (J, cin, 1, 1) and b.shape == (J,) and w.dtype == b.dtype == torch.float32 and w.is_cuda
    wt32 = np.concatenate([w.cpu().numpy().reshape(J, cin), b.cpu().numpy()[:, None]], 1)
    q = ref.normal64(p.feat, p.target, p.tw, cin, True, drawn=p.drawn)
    _, lmax = ref.solve64(q.A, q.r, q.n)
    b_g = ref.bound_g(q, wt32, lmax)
    g64 = hf.head_grad64(p.feat, wt32[:, :cin], wt32[:, cin], p.target, p.tw, True, drawn=p.drawn)
    g = np.concatenate([g64.dw, g64.db[:, None]], 1)
    print("%s: float64 gradient at the solved fp32 head: max |g| %.3g, max |g| / B_g %.3g" % (shape, np.abs(g).max(), (np.abs(g) / np.maximum(b_g, 1e-300)).max()))
    assert (np.abs(g) <= b_g).all()
    fit = acc.head_fit()
    assert torch.equal(fit.weight.detach(), w) and torch.equal(fit.bias.detach(), b)
    feat = up(np.nan_to_num(p.feat), np.float32)
    kw = dict(joints_hm=p.mu, joints_vis=p.vis, joints_weight=p.jw)
    gd = fit.grad(feat, **kw)
    dw = np.abs(gd.dw.cpu().numpy())
    print("%s: head_grad at the solved head: max |dw| / (B_g + B_dw) %.3g" % (shape, (dw / np.maximum(b_g[:, :cin] + g64.b_dw, 1e-300)).max()))
    assert (dw <= b_g[:, :cin] + g64.b_dw).all() and (np.abs(gd.db.cpu().numpy()) <= b_g[:, cin] + g64.b_db).all()
    at = acc.loss(w, b)
    state_b = ref.bound_loss(q, wt32)
    print("%s: loss at the solution %.17g (state) %.17g (head_grad), |diff| %.3g, bound %.3g + %.3g" % (shape, at, gd.loss.item(), abs(at - gd.loss.item()), g64.b_loss, state_b))
    assert abs(at - gd.loss.item()) <= g64.b_loss + state_b
    assert at <= acc.loss(p.w[:, :cin], p.b)
    rng = np.random.default_rng(11)
    for _ in range(6):
        d = rng.standard_normal(wt32.shape) * 1e-2 * max(np.abs(wt32).max(), 1e-3)
        assert at <= acc.loss(wt32[:, :cin] + d[:, :cin], wt32[:, cin] + d[:, cin])
    if shape == (2, 14, 8, 8, 16):
        assert not wt32[5].any(), "a joint that is never visible: zero weights, zero bias"
    # ridge: the weights shrink, the penalised gradient stays inside the bound (its own rounding included)
    wr, br = acc.solve(ridge=1e-3)
    assert (wr.double() ** 2).sum().item() <= (w.double() ** 2).sum().item()
    wr32 = np.concatenate([wr.cpu().numpy().reshape(J, cin), br.cpu().numpy()[:, None]], 1)
    gr = hf.head_grad64(p.feat, wr32[:, :cin], wr32[:, cin], p.target, p.tw, True, drawn=p.drawn)
    pen = 1e-3 * wr32[:, :cin].astype(np.float64)
    lam_r = lmax + 1e-3 * q.n * J
    b_gr = ref.bound_g(q, wr32, lam_r) + np.concatenate([hf.U * np.abs(pen), np.zeros((J, 1))], 1)
    assert (np.abs(np.concatenate([gr.dw + pen, gr.db[:, None]], 1)) <= b_gr).all()


def test_splitting_merging_and_an_invisible_crop():
    p = ref.shape_problem((3, 17, 17, 13, 80))
    feat = up(np.nan_to_num(p.feat), np.float32)
    kw = lambda s: dict(joints_hm=p.mu[s], joints_vis=p.vis[s], joints_weight=p.jw)
    whole = caller.HeadSolve(78, p.J, device=dev()).add(feat, **kw(slice(None)))
    split = caller.HeadSolve(78, p.J, device=dev()).add(feat[:1], **kw(slice(0, 1))).add(feat[1:], **kw(slice(1, 3)))
    a, b = caller.HeadSolve(78, p.J, device=dev()).add(feat[:2], **kw(slice(0, 2))), caller.HeadSolve(78, p.J, device=dev()).add(feat[2:], **kw(slice(2, 3)))
    merged = a.merge(b)
    for other in (split, merged):
        for x, y in zip(whole.state[:3], other.state[:3]):
            scale = x.abs().max().item()
            assert (x - y).abs().max().item() <= 1e-12 * scale
        assert torch.equal(whole.state.n, other.state.n)
    with pytest.raises(ValueError):
        whole.merge(caller.HeadSolve(64, p.J, device=dev()))
    vis = p.vis.copy()
    vis[2] = 0
    three = caller.HeadSolve(78, p.J, device=dev()).add(feat, joints_hm=p.mu, joints_vis=vis, joints_weight=p.jw)
    two = caller.HeadSolve(78, p.J, device=dev()).add(feat[:2], **kw(slice(0, 2)))
    assert all(torch.equal(x, y) for x, y in zip(three.state[:3], two.state[:3])), "a crop whose joints are all invisible changes only n"
    assert three.state.n.item() == 3 * 17 * 13 and two.state.n.item() == 2 * 17 * 13


def test_end_to_end_on_the_models_own_heat_maps():
    """minimality: with the model's heat maps as target the solved head cannot lose to the model's own head"""
    e = e2e()
    S, J, h, w = e.y.shape
    cin = e.hi.cin
    acc = caller.HeadSolve(cin, J, cfg=e.cfg).add(e.hi.feat, e.y, torch.ones(S, J, device=e.y.device))
    w_own, b_own = e.sd["final_layer.weight"], e.sd["final_layer.bias"]
    ws, bs = acc.solve()
    own, solved = acc.loss(w_own, b_own), acc.loss(ws, bs)
    q = ref.normal64(e.hi.feat.cpu().numpy(), e.y.cpu().numpy(), np.ones((S, J), np.float32), cin, True)
    cat = lambda a, b: np.concatenate([a.detach().cpu().numpy().reshape(J, cin), b.detach().cpu().numpy().reshape(J, 1)], 1)
    bound = ref.bound_loss(q, cat(w_own, b_own)) + ref.bound_loss(q, cat(ws, bs))
    diff = (caller.head_apply(e.hi.feat, ws, bs) - e.y).abs().max().item()
    print("own heat maps as target: loss of the model's head %.6g, of the solved head %.6g, bounds %.3g; head_apply(solution) against the heat maps: max |diff| %.3g"
          % (own, solved, bound, diff))
    assert solved <= own + bound


def test_end_to_end_the_solution_beats_ten_gradient_steps_and_commits():
    e = e2e()
    S, J, h, w = e.y.shape
    cin, N = e.hi.cin, S * h * w
    mu, vis = _targets(e)
    sigma = e.cfg.MODEL.SIGMA
    _, tw = _val_ref.joint_targets(mu, vis, h, w, sigma)
    f = e.hi.feat.cpu().numpy()
    ft = np.concatenate([f[..., :cin].astype(np.float64).reshape(S, h * w, cin), np.ones((S, h * w, 1))], 2)
    A = np.einsum("spa,spb->sab", ft, ft)
    L = max(float(np.linalg.eigvalsh(np.einsum("s,sab->ab", tw[:, j].astype(np.float64) ** 2, A) / (N * J))[-1]) for j in range(J))
    fit = caller.HeadFit(cin, J, torch.zeros(J, cin, 1, 1), torch.zeros(J), optimizer=lambda ps: torch.optim.SGD(ps, lr=1.0 / L))
    for step in range(10):
        fit.step(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma)
    after_steps = fit.grad(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma).loss.item()
    acc = caller.HeadSolve(cin, J).add(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma)
    solved = acc.head_fit()
    after_solve = solved.grad(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma).loss.item()
    print("loss after ten 1 / L steps from zero %.6g, after solve() %.6g (from the state %.6g)" % (after_steps, after_solve, acc.loss(solved.weight, solved.bias)))
    assert after_solve <= after_steps
    net = models.interformer.get_pose_net(e.cfg, is_train=False)
    net.load_state_dict(e.sd, strict=True)
    net = net.cuda()
    solved.commit(net)
    st = net.state_dict()
    assert torch.equal(st["final_layer.weight"], solved.weight.detach()) and torch.equal(st["final_layer.bias"], solved.bias.detach())
    y = multi(net(e.x, e.m, e.length))
    assert torch.equal(y, caller.head_apply(e.hi.feat, solved.weight, solved.bias))
    assert set(solved.state()) == {"final_layer.weight", "final_layer.bias"}
    solved.step(e.hi.feat, joints_hm=mu, joints_vis=vis, sigma=sigma)      # further steps work unchanged


def test_add_runs_without_a_host_synchronisation(monkeypatch):
    p = ref.shape_problem((3, 17, 7, 5, 32))
    feat = up(np.nan_to_num(p.feat), np.float32)
    hm, vis = up(p.mu, np.float64), up(p.vis, np.float32)
    target, tw = up(p.target, np.float32), up(p.tw, np.float32)
    acc = caller.HeadSolve(32, p.J, device=dev())
    syncs = []
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: syncs.append("cpu") or self.to("cpu"))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: syncs.append("item") or self.tolist())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.append("synchronize"))
    acc.add(feat, joints_hm=hm, joints_vis=vis)
    acc.add(feat, target, tw)
    caller.head_normal(feat, target, tw, cin=32)
    assert syncs == []


def test_no_crops_and_bad_arguments_are_codes_not_launches():
    p = ref.shape_problem((3, 17, 7, 5, 32))
    J = p.J
    ok = dict(target=p.target, tw=p.tw)
    z = np.zeros((0, p.h, p.w_, 36), np.float32)
    assert not run_normal(z, J, 32, target=np.zeros((0, J, p.h, p.w_), np.float32), tw=np.zeros((0, J), np.float32)).touched, "n_crops == 0 touches nothing"
    assert not run_normal(z, J, 32, mu=np.zeros((0, J, 2)), vis=np.zeros((0, J), np.float32)).touched
    assert not run_normal(p.feat, 33, 32, target=np.zeros((p.S, 33, p.h, p.w_), np.float32), use_w=False, expect=-1).touched
    big = np.zeros((p.S, p.h, p.w_, 148), np.float32)
    for cin in (24, 144, 0):
        assert not run_normal(big, J, cin, cin_out=16, expect=-1, **ok).touched, cin
    assert not run_normal(p.feat, J, 32, mu=p.mu, vis=p.vis, expect=-1, **ok).touched, "both target forms"
    r = run_normal(p.feat, J, 32, expect=-1)
    assert not r.touched and b"target form" in cabi.lib().i2r_last_error(), "neither target form"
    assert not run_normal(p.feat, J, 32, feat_offset=1, expect=-1, **ok).touched, "feat off its 16-byte boundary"
    assert not run_normal(p.feat, J, 32, target=p.target, expect=-1).touched, "a weighted loss without weights"
    assert not run_normal(p.feat, J, 32, mu=p.mu, expect=-1).touched, "the analytic form without joints_vis"
    for bad in (dict(in_cs=28), dict(in_cs=34), dict(h=0), dict(n_crops=-1), dict(joints=0), dict(A=None), dict(n=None), dict(ws=None), dict(cin_out=0),
                dict(cin_out=33), dict(ld=32)):
        assert not run_normal(p.feat, J, 32, expect=-1, **ok, **bad).touched, bad
    assert not run_normal(p.feat, J, 32, mu=p.mu, vis=p.vis, sigma=0.0, expect=-1).touched
    # the Python surface
    ft = torch.zeros(0, p.h, p.w_, 16, device=dev())
    s = caller.head_normal(ft, joints_hm=np.zeros((0, J, 2)), joints_vis=np.zeros((0, J)))
    assert s.A.shape == (J, 17, 17) and not s.A.any() and s.n.item() == 0
    with pytest.raises(cabi.I2RError):
        caller.head_normal(torch.zeros(1, 4, 4, 16, device=dev()))
    with pytest.raises(cabi.I2RError):
        caller.head_normal(torch.zeros(1, 4, 4, 16, device=dev()), torch.zeros(1, 2, 4, 4, device=dev()), torch.ones(1, 2), cin=30)
