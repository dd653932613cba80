"""CPU: the float64 reference of the head re-fit's normal equations (tests/_head_solve_ref.py) against the stacked weighted least-squares
system and against the gradient reference of tests/_head_fit_ref.py; the derived bounds against a numpy emulation of the kernel's fp32
arithmetic -- the emulation stays inside them, and tw in place of tw^2, a dropped pixel and a missing bias row each leave them; the C-ABI
surface of i2r_head_normal."""
import ctypes
import os
import re

import numpy as np
import pytest

import _head_fit_ref as hf
import _head_solve_ref as ref
from i2r_amd import cabi, caller
from test_val_metrics import _c_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTION = 0.25      # the emulation's chains are a whole crop long, the worst the kernel can have; random roundings stay far below the
                     # worst case the bound is built for -- a quarter of it is the room the issue's own check (0.13, 0.11) leaves


def stacked(p, j, use_w):
    """joint j's weighted least-squares system: rows tw f~, right-hand side tw t"""
    S, hw = p.S, p.h * p.w_
    Ft = ref._ft(p.feat, p.cin, np.float64)
    tw = p.tw[:, j].astype(np.float64) if use_w else np.ones(S)
    M = (tw[:, None, None] * Ft).reshape(S * hw, p.cin + 1)
    y = (tw[:, None] * p.target[:, j].reshape(S, hw).astype(np.float64)).reshape(-1)
    return M, y


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_reference_is_the_stacked_least_squares_system_and_solves_it(shape):
    p = ref.shape_problem(shape, seed=1, pad=0)
    for use_w in (True, False):
        q = ref.normal64(p.feat, p.target, p.tw, p.cin, use_w)
        assert q.n == p.S * p.h * p.w_
        wt, _ = ref.solve64(q.A, q.r, q.n)
        mine = caller.solve_normal(q.A, q.r, q.n)
        assert np.array_equal(mine, wt), "caller.solve_normal is the same arithmetic"
        full = 0
        for j in range(p.J):
            M, y = stacked(p, j, use_w)
            scale = max(np.abs(M.T @ M).max(), 1.0)
            assert np.abs(q.A[j] - M.T @ M).max() <= 1e-12 * scale and np.abs(q.r[j] - M.T @ y).max() <= 1e-12 * max(np.abs(M.T @ y).max(), 1.0)
            assert abs(q.c[j] - y @ y) <= 1e-12 * max(y @ y, 1.0)
            sv = np.linalg.svd(M, compute_uv=False)
            if sv[-1] > 1e-6 * sv[0] and M.shape[0] >= M.shape[1]:     # full rank: the normal equations lose cond^2 eps, here <= 1e-4
                full += 1
                w_ls = np.linalg.lstsq(M, y, rcond=None)[0]
                tol = 1e3 * 2.0 ** -52 * (sv[0] / sv[-1]) ** 2 * max(np.abs(w_ls).max(), 1e-30)
                assert np.abs(wt[j] - w_ls).max() <= tol, (j, np.abs(wt[j] - w_ls).max(), tol)
        print("shape %s use_w %d: %d of %d joints of full rank" % (shape, use_w, full, p.J))
        if shape[0] * shape[2] * shape[3] > 2 * (shape[4] + 1) and shape[4] != 80:
            assert full > 0


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_gradient_vanishes_at_the_solution_and_the_loss_comes_from_the_state(shape):
    p = ref.shape_problem(shape, seed=2, pad=0)
    cin, J = p.cin, p.J
    for use_w in (True, False):
        q = ref.normal64(p.feat, p.target, p.tw, cin, use_w)
        start = hf.head_grad64(p.feat, p.w, p.b, p.target, p.tw, use_w)
        g0 = max(np.abs(start.dw).max(), np.abs(start.db).max())
        wt, _ = ref.solve64(q.A, q.r, q.n)
        at = hf.head_grad64(p.feat, wt[:, :cin], wt[:, cin], p.target, p.tw, use_w)
        g1 = max(np.abs(at.dw).max(), np.abs(at.db).max())
        print("shape %s use_w %d: |grad| at the start %.3g, at the solution %.3g; loss %.6g -> %.6g" % (shape, use_w, g0, g1, start.loss, at.loss))
        assert g1 <= 1e-10 * g0
        assert np.abs(ref.grad64(q.A, q.r, q.n, wt)).max() <= 1e-10 * g0
        # the gradient from the state is head_grad64's
        gs = ref.grad64(q.A, q.r, q.n, np.concatenate([p.w, p.b[:, None]], 1))
        assert np.abs(gs[:, :cin] - start.dw).max() <= 1e-12 * g0 and np.abs(gs[:, cin] - start.db).max() <= 1e-12 * g0
        for w_, l_ in ((np.concatenate([p.w, p.b[:, None]], 1), start.loss), (wt, at.loss)):
            got = ref.loss64(q.A, q.r, q.c, q.n, w_)
            assert abs(got - l_) <= 1e-12 * max(abs(start.loss), abs(l_)), (got, l_)
        assert at.loss <= start.loss
        # ridge: the gradient of L + ridge / 2 ||W||^2 vanishes, the bias is not penalised, the weights shrink
        ridge = 1e-3
        wr, _ = ref.solve64(q.A, q.r, q.n, ridge=ridge)
        gr = hf.head_grad64(p.feat, wr[:, :cin], wr[:, cin], p.target, p.tw, use_w)
        assert np.abs(gr.dw + ridge * wr[:, :cin]).max() <= 1e-10 * g0 and np.abs(gr.db).max() <= 1e-10 * g0
        assert (wr[:, :cin] ** 2).sum() <= (wt[:, :cin] ** 2).sum() * (1 + 1e-12)
    q = ref.normal64(p.feat, p.target, p.tw, cin, True)
    wt, _ = ref.solve64(q.A, q.r, q.n)
    if shape == (2, 14, 8, 8, 16):
        assert not q.A[5].any() and not wt[5].any(), "a joint that is never visible gets zero weights and zero bias"
    if cin == 80:
        assert np.abs(wt[:, 78:80]).max() <= 1e-12 * np.abs(wt).max(), "dead channels: the minimum-norm minimiser leaves them at zero"


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_fp32_emulation_stays_inside_the_bounds_and_three_defects_leave_them(shape):
    p = ref.shape_problem(shape, seed=3, pad=0)
    S, hw, cin = p.S, p.h * p.w_, p.cin
    for use_w in (True, False):
        q = ref.normal64(p.feat, p.target, p.tw, cin, use_w)
        e = ref.excess(ref.emulate32(p.feat, p.target, p.tw, cin, use_w), q)
        print("shape %s use_w %d: emulation / bound (A, r, c) %s" % (shape, use_w, ["%.3g" % v for v in e]))
        assert max(e) <= FRACTION
        qa = ref.normal64(p.feat, p.target, p.tw, cin, use_w, drawn=p.drawn)
        assert (qa.b_r >= q.b_r).all() and np.array_equal(qa.b_A, q.b_A)
        # the pixel with the largest feature of a crop that carries weight
        mag = np.abs(p.feat[..., :cin].reshape(S, hw, cin)).max(2) * ((p.tw.max(1) > 0) | (not use_w))[:, None]
        drop = np.unravel_index(np.argmax(mag), mag.shape)
        for defect in ("tw", "drop", "bias"):
            if defect == "tw" and not use_w:
                continue
            d = ref.excess(ref.emulate32(p.feat, p.target, p.tw, cin, use_w, defect=defect, drop=drop), q)
            print("shape %s use_w %d: defect %-4s / bound (A, r, c) %s" % (shape, use_w, defect, ["%.3g" % v for v in d]))
            assert d[0] > 1.0, (defect, d)
            if defect != "drop":     # (the dropped pixel's targets may all be zero: then r does not see it)
                assert d[1] > 1.0, (defect, d)


def test_header_binding_and_exports_agree_and_abi_stays_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    assert re.search(r"^I2R_API\s+int\s+i2r_head_normal\s*\(const i2r_head_normal_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"^I2R_API\s+int\s+i2r_head_normal_ws_bytes\s*\(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t\* bytes\);",
                     header, flags=re.M)
    assert "i2r_head_normal" in cabi.EXPORTS and "i2r_head_normal_ws_bytes" in cabi.EXPORTS
    assert _c_struct_fields(header, "i2r_head_normal_args") == [(n, t) for n, t in cabi.HeadNormalArgs._fields_]
    assert ctypes.sizeof(cabi.HeadNormalArgs) == 11 * 8 + 8 + 10 * 4
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    exported = __graft_entry__.exported_symbols(cabi.LIB_PATH)
    assert "i2r_head_normal" in exported and "i2r_head_normal_ws_bytes" in exported
    assert "i2r_head_fit.hip" in __graft_entry__.SOURCES and len(__graft_entry__.SOURCES) == 22, "the source list of the build does not change"


def test_workspace_size_is_a_function_of_the_shape_and_bad_shapes_are_codes():
    """no GPU: the size query computes, it launches nothing"""
    L = cabi.load_library()
    n, m = ctypes.c_int64(-1), ctypes.c_int64(-2)
    assert L.i2r_head_normal_ws_bytes(32, 64, 48, 96, 17, ctypes.byref(n)) == 0 and L.i2r_head_normal_ws_bytes(32, 64, 48, 96, 17, ctypes.byref(m)) == 0
    assert n.value == m.value > 0 and n.value % 4 == 0
    assert n.value >= 32 * (21 * 256 * 4 + 17 * 96 * 4), "at least one part per crop: its 21 Gram tiles and its share of r"
    assert n.value < 38 * 2 ** 20 // 2, "the partials stay well below the one read of the features (38 MB)"
    assert L.i2r_head_normal_ws_bytes(0, 64, 48, 96, 17, ctypes.byref(n)) == 0 and n.value == 0
    for bad in ((1, 8, 8, 24, 17), (1, 8, 8, 144, 17), (1, 8, 8, 96, 33), (1, 8, 8, 96, 0), (1, 0, 8, 96, 17), (-1, 8, 8, 96, 17)):
        assert L.i2r_head_normal_ws_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert L.i2r_head_normal_ws_bytes(1, 8, 8, 96, 17, None) == -1
    a = cabi.HeadNormalArgs()
    assert L.i2r_head_normal(None, None) == -1 and L.i2r_head_normal(ctypes.byref(a), None) == -1
