"""float64 reference of i2r_head_normal (include/i2r_hip.h): the normal equations of JointsMSELoss in (W, b) on frozen features, the
bounds the device state must meet, the closed-form solve, and a numpy emulation of the kernel's fp32 arithmetic that
tests/test_head_solve.py holds against those bounds on the CPU.

The bounds, with u = 2^-24 and starred quantities from float64 (the fp32 matrix pipe is bitwise an fmaf chain).  The kernel's order:
a part (a run of 16-pixel fragments of ONE crop) accumulates its Gram tiles and its share of r as fp32 fma chains over its pixels, the
column sums F^T 1 as fp32 additions (a lane adds every fourth pixel: a chain of at most h w / 4 additions); everything else is float64.
So the longest fp32 chain is k <= h w, and
  B_A[j,a,b] = (k + 2) u sum_s tw^2 sum_p |f~_a||f~_b| + delta_A     (chain k; tw^2 is exact in float64; the 2 is slack)
  B_r[j,a]   = sum_s sum_p (tw^2 e_t + (k + 4) u |tw^2 t|) |f~_a| + delta_r
                                                                    (chain k, the roundings of tw * tw and of (tw tw) * t, e_t = 2.5e-7
                                                                    for a drawn analytic target)
  B_c[j]     = the B_sse of _head_fit_ref at o = 0                    (c is i2r_head_grad's sse at W = 0, b = 0)
  delta      = (parts per crop + S + 16) 2^-53 times the same sum of absolute values: the float64 additions of the finish launch (a
               crop's parts, the crops of a slice, the 32 slices, the product with tw^2, state += sum); parts per crop <= ceil(h w / 16)
  B_g[j,a]   = (sum_b B_A[j,a,b] |w~_b| + B_r[j,a] + u sum_b |A*_ab||w~_b| + rcond lmax_j ||w~_j|| + 8 (cin + 1) 2^-52 lmax_j ||w~_j||) / (n J)
               the gradient at the solved fp32 head: the state's error, the one rounding of the solution to fp32, the directions
               dropped at rcond, and the float64 solve -- a symmetric eigendecomposition (backward error a modest multiple of
               (cin + 1) eps ||A||, taken as 4) and two products with the eigenvector matrix ((cin + 1) eps ||A|| ||w~|| each, taken as 2 + 2)"""
import types

import numpy as np

import _head_fit_ref as hf
import _val_ref

U = hf.U
E_T = hf.E_T

# (S, J, h, w, cin): the smallest shapes at which the kernel can go wrong (one fragment and fewer pixels than unknowns; 35 pixels and two
# joint fragments; a joint that is never visible; 78 non-zero channels of 80; the weighted and unweighted forms at cin 96; both maxima)
SHAPES = [(1, 1, 4, 4, 16), (3, 17, 7, 5, 32), (2, 14, 8, 8, 16), (3, 17, 17, 13, 80), (3, 20, 16, 12, 96), (2, 32, 16, 8, 128)]


def shape_problem(shape, seed=0, pad=4):
    """hf.problem at that shape with in_cs = cin + pad and NaN behind cin (the kernel must not read there); cin 80: 78 non-zero channels;
    (2, 14, 8, 8, 16): joint 5 is never visible"""
    S, J, h, w, cin = shape
    p = hf.problem(S, J, h, w, cin, seed=seed, cs=cin + pad, nonzero=78 if cin == 80 else None)
    if pad:
        p.feat[..., cin:] = np.nan
    if shape == (2, 14, 8, 8, 16):
        p.vis[:, 5] = 0
        p.target, p.tw = _val_ref.joint_targets(p.mu, p.vis, h, w, 2, p.jw)
        p.drawn = _val_ref.joint_targets(p.mu, p.vis, h, w, 2, None)[1] > 0.5
        assert not p.tw[:, 5].any()
    return p


def _ft(feat, cin, dtype):
    S, h, wd, _ = feat.shape
    F = np.asarray(feat)[..., :cin].astype(dtype).reshape(S, h * wd, cin)
    return np.concatenate([F, np.ones((S, h * wd, 1), dtype)], 2)


def normal64(feat, target, tw, cin, use_w=True, drawn=None, u=U):
    """feat [S, h, w, >= cin] fp32, target [S, J, h, w], tw [S, J]; drawn: bool [S, J] (None: tensor form, e_t = 0)
    -> namespace A [J, cin + 1, cin + 1], r [J, cin + 1], c [J], n and the bounds b_A, b_r, b_c"""
    S, h, wd, _ = feat.shape
    J = np.asarray(tw).shape[1]
    hw = h * wd
    Ft = _ft(feat, cin, np.float64)
    t = np.asarray(target, np.float64).reshape(S, J, hw)
    twv = np.asarray(tw, np.float64).reshape(S, J) if use_w else np.ones((S, J))
    tw2 = twv * twv
    q = types.SimpleNamespace(n=S * hw, J=J, cin=cin)
    q.A = np.einsum("sj,sab->jab", tw2, np.einsum("spa,spb->sab", Ft, Ft))
    q.r = np.einsum("sj,sjp,spa->ja", tw2, t, Ft)
    z = hf.head_grad64(feat, np.zeros((J, cin)), np.zeros(J), target, tw, use_w, drawn=drawn, u=u)
    q.c, q.b_c = z.sse, z.b_sse
    aF = np.abs(Ft)
    absA = np.einsum("sj,sab->jab", tw2, np.einsum("spa,spb->sab", aF, aF))
    e_t = np.zeros((S, J)) if drawn is None else np.where(np.asarray(drawn, bool), E_T, 0.0)
    absr = np.einsum("sj,sjp,spa->ja", tw2, np.abs(t), aF)
    delta = ((hw + 15) // 16 + S + 16) * 2.0 ** -53
    q.b_A = (hw + 2) * u * absA + delta * absA
    q.b_r = np.einsum("sj,spa->ja", tw2 * e_t, aF) + (hw + 4) * u * absr + delta * absr
    q.absA = absA
    return q


def default_rcond(cin):
    return (cin + 1) * 2.0 ** -52


def solve64(A, r, n, ridge=0.0, rcond=None):
    """per joint the minimum-norm solution of (A_j + ridge n J diag(1 .. 1, 0)) w~ = r_j by a symmetric eigendecomposition that drops
    eigenvalues <= rcond lmax -> (w~ [J, cin + 1] float64, lmax [J])"""
    J, m, _ = A.shape
    rcond = default_rcond(m - 1) if rcond is None else rcond
    pen = np.ones(m)
    pen[-1] = 0
    wt, lmax = np.zeros((J, m)), np.zeros(J)
    for j in range(J):
        lam, V = np.linalg.eigh(A[j] + ridge * n * J * np.diag(pen))
        lmax[j] = max(float(lam[-1]), 0.0)
        keep = lam > rcond * lmax[j]
        wt[j] = V[:, keep] @ ((V[:, keep].T @ r[j]) / lam[keep])
    return wt, lmax


def loss64(A, r, c, n, wt):
    """L(W, b) = (1 / (2 n J)) sum_j (w~^T A w~ - 2 w~^T r + c) in float64"""
    J = A.shape[0]
    wt = np.asarray(wt, np.float64)
    return float((np.einsum("ja,jab,jb->j", wt, A, wt) - 2 * (wt * r).sum(1) + c).sum() / (2.0 * n * J))


def grad64(A, r, n, wt, ridge=0.0):
    """the gradient of L + ridge / 2 ||W||^2 at w~ [J, cin + 1], from the state -> [J, cin + 1]"""
    J = A.shape[0]
    wt = np.asarray(wt, np.float64)
    g = (np.einsum("jab,jb->ja", A, wt) - r) / (n * J)
    g[:, :-1] += ridge * wt[:, :-1]
    return g


def bound_g(q, wt32, lmax, rcond=None, u=U):
    """B_g [J, cin + 1] at the fp32 head wt32 (module docstring); q = normal64(...) of everything accumulated"""
    w = np.abs(np.asarray(wt32, np.float64))
    rcond = default_rcond(q.cin) if rcond is None else rcond
    nrm = np.sqrt((w * w).sum(1))[:, None]
    solve = (rcond + 8 * (q.cin + 1) * 2.0 ** -52) * lmax[:, None] * nrm
    return (np.einsum("jab,jb->ja", q.b_A, w) + q.b_r + u * np.einsum("jab,jb->ja", np.abs(q.A), w) + solve) / (q.n * q.J)


def bound_loss(q, wt):
    """what the state's error can move L(W, b) by: (w~^T B_A w~ + 2 |w~|^T B_r + B_c) / (2 n J)"""
    w = np.abs(np.asarray(wt, np.float64))
    return float((np.einsum("ja,jab,jb->j", w, q.b_A, w) + 2 * (w * q.b_r).sum(1) + q.b_c).sum() / (2.0 * q.n * q.J))


def emulate32(feat, target, tw, cin, use_w=True, defect=None, drop=None):
    """The kernel's arithmetic in numpy fp32, with the longest chains it can have: per crop the Gram matrix and r as fma chains over ALL
    the crop's pixels, the column sums as fp32 additions, tw^2 t rounded as tw * tw, then * t; float64 across crops with tw^2 exact.
    defect: None | "tw" (tw in place of tw^2) | "drop" (pixel drop = (s, p) left out of A and r) | "bias" (no bias row and column)
    -> namespace A, r, c (float64), n"""
    S, h, wd, _ = feat.shape
    J = np.asarray(tw).shape[1]
    hw = h * wd
    F = np.asarray(feat, np.float32)[..., :cin].reshape(S, hw, cin)
    t = np.asarray(target, np.float32).reshape(S, J, hw)
    twv = np.asarray(tw, np.float32).reshape(S, J) if use_w else np.ones((S, J), np.float32)
    tw2 = twv if defect == "tw" else twv * twv
    assert tw2.dtype == np.float32
    gt = tw2[:, :, None] * t
    assert gt.dtype == np.float32
    G = np.zeros((S, cin, cin), np.float32)
    cs = np.zeros((S, cin), np.float32)
    racc = np.zeros((S, J, cin), np.float32)
    live = np.ones((S, hw), bool)
    if defect == "drop":
        live[drop[0], drop[1]] = False
    for p in range(hw):
        m = live[:, p]
        G[m] = hf._fma32(F[m, p, :, None], F[m, p, None, :], G[m])
        cs[m] = (cs[m] + F[m, p]).astype(np.float32)
        racc[m] = hf._fma32(gt[m, :, p, None], F[m, p, None, :], racc[m])
    w2 = (twv.astype(np.float64) if defect == "tw" else twv.astype(np.float64) ** 2)
    q = types.SimpleNamespace(n=S * hw, J=J, cin=cin)
    Gt = np.zeros((S, cin + 1, cin + 1))
    Gt[:, :cin, :cin] = G
    rb = (gt.astype(np.float64) * live[:, None, :]).sum(2)
    if defect != "bias":
        Gt[:, :cin, cin] = Gt[:, cin, :cin] = cs
        Gt[:, cin, cin] = live.sum(1)
    else:
        rb = rb * 0
    q.A = np.einsum("sj,sab->jab", w2, Gt)
    q.r = np.concatenate([racc.astype(np.float64).sum(0), rb.sum(0)[:, None]], 1)
    d = t * twv[:, :, None]
    assert d.dtype == np.float32
    q.c = (d * d).astype(np.float64).sum((0, 2))
    return q


def excess(got, ref):
    """max |got - ref| / bound over A, r, c -> (A, r, c): <= 1 means inside the bound"""
    def ratio(a, b, bound):
        diff = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
        return float(np.max(np.where(diff == 0, 0.0, diff / np.where(bound > 0, bound, np.finfo(np.float64).tiny))))
    return ratio(got.A, ref.A, ref.b_A), ratio(got.r, ref.r, ref.b_r), ratio(got.c, ref.c, ref.b_c)
