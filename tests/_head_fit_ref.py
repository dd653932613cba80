"""float64 reference of i2r_head_grad (include/i2r_hip.h) with the bound its outputs must meet, and a numpy emulation of the kernel's
fp32 arithmetic that tests/test_head_fit.py holds against that bound on the CPU.

The bound, with u = 2^-24 and starred quantities from float64 (the fp32 matrix pipe is bitwise an fmaf chain):
  per (s, j, p)   e_o = (cin + 1) u (sum_c |w||f| + |b|)         the chain of cin fmas that starts at the bias
                  e_t = 2.5e-7 for a drawn analytic target (the header's distance of the in-kernel Gaussian), else 0
                  e_g = tw^2 (e_o + e_t) + 4 u |g*|               tw * tw, o - t, their product
  per output      B_dw[j, c] = (sum e_g |f| + (h w + 4) u sum |g*||f|) / (N J) + u |dw*|
                                                                  an fp32 accumulator holds at most one crop's h w pixels; the rest is
                                                                  float64; one division, one rounding to fp32
                  B_db the same with |f| -> 1
                  B_loss = sum (|tw d*| tw (e_o + e_t) + 4 u (tw d*)^2) / (N J),  d* = o* - t
                  B_sse[j] = 2 N J times joint j's share of B_loss (loss = sum_j 0.5 sse[j] / (N J))"""
import types

import numpy as np

U = 2.0 ** -24
E_T = 2.5e-7


def head_grad64(feat, w, b, target, tw, use_w=True, drawn=None, u=U):
    """feat [S, h, w, >= cin] fp32, w [J, cin] (cin = w.shape[1]: hand in exactly the columns the kernel is told to read), b [J],
    target [S, J, h, w], tw [S, J]; drawn: bool [S, J], the analytic targets that are drawn (None: tensor form, e_t = 0).
    -> namespace: o, g, dw, db, loss, sse (float64) and the bounds b_dw, b_db, b_loss, b_sse, e_o"""
    S, h, wd, _ = feat.shape
    J, cin = w.shape
    hw, N = h * wd, S * h * wd
    F = np.asarray(feat, np.float64)[..., :cin].reshape(S, hw, cin)
    W, B = np.asarray(w, np.float64), np.asarray(b, np.float64)
    t = np.asarray(target, np.float64).reshape(S, J, hw)
    twv = np.asarray(tw, np.float64).reshape(S, J, 1) if use_w else np.ones((S, J, 1))
    r = types.SimpleNamespace()
    r.o = np.einsum("spc,jc->sjp", F, W) + B[None, :, None]
    d = r.o - t
    x = twv * d
    r.sse = (x * x).sum((0, 2))
    r.loss = float((0.5 * r.sse / N).sum() / J)
    r.g = twv * twv * d
    r.dw = np.einsum("sjp,spc->jc", r.g, F) / (N * J)
    r.db = r.g.sum((0, 2)) / (N * J)
    aF = np.abs(F)
    r.e_o = (cin + 1) * u * (np.einsum("spc,jc->sjp", aF, np.abs(W)) + np.abs(B)[None, :, None])
    e_t = np.zeros((S, J, 1)) if drawn is None else np.where(np.asarray(drawn, bool), E_T, 0.0).reshape(S, J, 1)
    e_g = twv * twv * (r.e_o + e_t) + 4 * u * np.abs(r.g)
    aG = np.abs(r.g)
    r.b_dw = (np.einsum("sjp,spc->jc", e_g, aF) + (hw + 4) * u * np.einsum("sjp,spc->jc", aG, aF)) / (N * J) + u * np.abs(r.dw)
    r.b_db = (e_g.sum((0, 2)) + (hw + 4) * u * aG.sum((0, 2))) / (N * J) + u * np.abs(r.db)
    per = np.abs(x) * twv * (r.e_o + e_t) + 4 * u * x * x
    r.b_sse = 2.0 * per.sum((0, 2))
    r.b_loss = float(per.sum() / (N * J))
    return r


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in float64; the sum is rounded there (2^-53) and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate32(feat, w, b, target, tw, use_w=True, defect=None, drop=None):
    """The kernel's arithmetic in numpy fp32: o as an fma chain over the channels that starts at the bias, g = (tw * tw) * (o - t), dW
    as an fma chain over ONE crop's pixels, float64 across crops, one division, one rounding.  target fp32 as the kernel would hold it.
    defect: None | "drop" (the g of pixel drop = (s, p) is left out) | "tw" (tw in place of tw^2) | "bias" (no bias)
    -> namespace dw, db (fp32), loss, sse (float64)"""
    S, h, wd, _ = feat.shape
    J, cin = w.shape
    hw, N = h * wd, S * h * wd
    F = np.asarray(feat, np.float32)[..., :cin].reshape(S, hw, cin)
    W = np.asarray(w, np.float32)
    t = np.asarray(target, np.float32).reshape(S, J, hw)
    twv = np.asarray(tw, np.float32).reshape(S, J, 1) if use_w else np.ones((S, J, 1), np.float32)
    o = np.broadcast_to(np.asarray(b, np.float32)[None, :, None], (S, J, hw)).copy()
    if defect == "bias":
        o[:] = 0
    for c in range(cin):
        o = _fma32(W[None, :, c, None], F[:, None, :, c], o)
    d = o * twv - t * twv
    assert d.dtype == np.float32
    sse = (d * d).astype(np.float64).sum((0, 2))
    g = (twv if defect == "tw" else twv * twv) * (o - t)
    assert g.dtype == np.float32
    if defect == "drop":
        g[drop[0], :, drop[1]] = 0
    acc = np.zeros((S, J, cin), np.float32)
    accb = np.zeros((S, J), np.float32)
    for p in range(hw):
        acc = _fma32(g[:, :, p, None], F[:, p, None, :], acc)
        accb = (accb + g[:, :, p]).astype(np.float32)
    r = types.SimpleNamespace()
    r.dw = (acc.astype(np.float64).sum(0) / (N * J)).astype(np.float32)
    r.db = (accb.astype(np.float64).sum(0) / (N * J)).astype(np.float32)
    r.sse = sse
    r.loss = float((0.5 * sse / N).sum() / J)
    return r


def excess(got, ref):
    """max over the outputs of |got - ref| / bound -> (dw, db, loss, sse): <= 1 means inside the bound"""
    def ratio(a, b, bound):
        a, b, bound = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(bound, np.float64)
        diff = np.abs(a - b)
        return float(np.max(np.where(diff == 0, 0.0, diff / np.where(bound > 0, bound, np.finfo(np.float64).tiny))))
    return (ratio(got.dw, ref.dw, ref.b_dw), ratio(got.db, ref.db, ref.b_db), ratio(got.loss, ref.loss, ref.b_loss), ratio(got.sse, ref.sse, ref.b_sse))


def problem(S, J, h, w, cin, seed=0, cs=None, nonzero=None):
    """a random head problem at that shape: features N(0, 1) (channels nonzero .. cin - 1 zero, the padding of a 78-channel model),
    weights N(0, 0.3^2 / cin), targets from random joints with visibilities 0 / 0.5 / 1 and a joints_weight table; map (0, 0) is a drawn
    joint of weight 1.2, so tw != tw^2 somewhere at every shape -> namespace"""
    import _val_ref
    rng = np.random.default_rng([seed, S, J, h, w, cin])
    cs = cin if cs is None else cs
    p = types.SimpleNamespace(S=S, J=J, h=h, w_=w, cin=cin, cs=cs)
    p.feat = rng.standard_normal((S, h, w, cs)).astype(np.float32)
    p.w = (rng.standard_normal((J, cin)) * 0.3 / np.sqrt(cin)).astype(np.float32)
    if nonzero is not None:
        p.feat[..., nonzero:] = 0
        p.w[:, nonzero:] = 0
    p.b = (rng.standard_normal(J) * 0.1).astype(np.float32)
    p.mu = np.floor(np.stack([rng.uniform(-2, w + 2, (S, J)), rng.uniform(-2, h + 2, (S, J))], 2)) + rng.choice([0.125, 0.25, 0.75], (S, J, 2))
    p.vis = rng.choice([0.0, 0.5, 1.0, 1.0], (S, J)).astype(np.float32)
    p.jw = (1.0 + 0.1 * (np.arange(J) % 4)).astype(np.float32)
    p.mu[0, 0], p.vis[0, 0], p.jw[0] = (w // 2 + 0.25, h // 2 + 0.25), 1.0, 1.2
    p.target, p.tw = _val_ref.joint_targets(p.mu, p.vis, h, w, 2, p.jw)
    _, tw_plain = _val_ref.joint_targets(p.mu, p.vis, h, w, 2, None)
    p.drawn = tw_plain > 0.5
    return p
