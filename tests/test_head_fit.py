"""CPU: the head re-fit's float64 reference (tests/_head_fit_ref.py) against torch float64 autograd through F.conv2d and the loss as
tests/_val_ref.py restates it; the derived bound against a numpy emulation of the kernel's fp32 arithmetic -- the emulation stays inside
it, and a dropped pixel, tw in place of tw^2 and a missing bias each leave it; the C-ABI surface of i2r_head_grad."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _head_fit_ref as ref
from i2r_amd import cabi, caller
from test_val_metrics import CASES, _c_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CINS = [16, 80, 96, 128, 96]      # one per case: the shapes x channel counts of the issue


def test_header_binding_and_exports_agree_and_abi_stays_17():
    import __graft_entry__
    header = open(os.path.join(ROOT, "include", "i2r_hip.h")).read()
    assert int(re.search(r"#define I2R_ABI_VERSION (\d+)", header).group(1)) == 17 == cabi.ABI_VERSION
    assert re.search(r"^I2R_API\s+int\s+i2r_head_grad\s*\(const i2r_head_grad_args\* a, void\* stream\);", header, flags=re.M)
    assert re.search(r"^I2R_API\s+int\s+i2r_head_grad_ws_bytes\s*\(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t\* bytes\);",
                     header, flags=re.M)
    assert "i2r_head_grad" in cabi.EXPORTS and "i2r_head_grad_ws_bytes" in cabi.EXPORTS
    assert _c_struct_fields(header, "i2r_head_grad_args") == [(n, t) for n, t in cabi.HeadGradArgs._fields_]
    assert ctypes.sizeof(cabi.HeadGradArgs) == 13 * 8 + 8 + 8 * 4
    if not os.path.exists(cabi.LIB_PATH):
        __graft_entry__.build()
    exported = __graft_entry__.exported_symbols(cabi.LIB_PATH)
    assert "i2r_head_grad" in exported and "i2r_head_grad_ws_bytes" in exported
    assert "i2r_head_fit.hip" in __graft_entry__.SOURCES
    src = open(os.path.join(ROOT, "intra-and-inter-human-relation-network-for-mpee_amd", "csrc", "i2r_metrics.hip")).read()
    assert '#include "i2r_targets.h"' in src and "float joint_weight(" not in src, "the target's definition is shared, not copied"


def test_workspace_size_is_a_function_of_the_shape_and_bad_shapes_are_codes():
    """no GPU: the size query computes, it launches nothing"""
    L = cabi.load_library()
    n = ctypes.c_int64(-1)
    assert L.i2r_head_grad_ws_bytes(32, 64, 48, 96, 17, ctypes.byref(n)) == 0
    per_part = 17 * 16 + 17 * 96 * 4
    assert n.value > 0 and n.value % per_part == 0 and n.value // per_part >= 32, "at least one part per crop"
    assert L.i2r_head_grad_ws_bytes(0, 64, 48, 96, 17, ctypes.byref(n)) == 0 and n.value == 0
    for bad in ((1, 8, 8, 24, 17), (1, 8, 8, 144, 17), (1, 8, 8, 96, 33), (1, 8, 8, 96, 0), (1, 0, 8, 96, 17), (-1, 8, 8, 96, 17)):
        assert L.i2r_head_grad_ws_bytes(*bad, ctypes.byref(n)) == -1, bad
    assert L.i2r_head_grad_ws_bytes(1, 8, 8, 96, 17, None) == -1
    a = cabi.HeadGradArgs()
    assert L.i2r_head_grad(None, None) == -1 and L.i2r_head_grad(ctypes.byref(a), None) == -1


def test_pad16_leaves_multiples_alone_and_pads_with_zero_columns():
    w = torch.arange(2 * 78, dtype=torch.float32).reshape(2, 78)
    p, c = caller._pad16(w, 78)
    assert c == 80 and p.shape == (2, 80) and torch.equal(p[:, :78], w) and (p[:, 78:] == 0).all()
    q, c = caller._pad16(p, 80)
    assert c == 80 and q is p


def _autograd64(p, use_w):
    """torch float64: F.conv2d on the NCHW features, the loss as _val_ref.val_metrics restates JointsMSELoss, autograd"""
    x = torch.from_numpy(p.feat[..., :p.cin].astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(p.w.astype(np.float64)).reshape(p.J, p.cin, 1, 1).requires_grad_()
    b = torch.from_numpy(p.b.astype(np.float64)).requires_grad_()
    out = F.conv2d(x, w, b)
    t = torch.from_numpy(p.target.astype(np.float64))
    tw = torch.from_numpy(p.tw.astype(np.float64)).reshape(p.S, p.J, 1, 1) if use_w else torch.ones(p.S, p.J, 1, 1, dtype=torch.float64)
    N = p.S * p.h * p.w_
    sse = ((out * tw - t * tw) ** 2).sum((0, 2, 3))
    loss = (0.5 * (sse / N)).sum() / p.J
    loss.backward()
    return loss.item(), sse.detach().numpy(), w.grad.reshape(p.J, p.cin).numpy(), b.grad.numpy()


@pytest.mark.parametrize("use_w", [1, 0])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_reference_is_the_gradient_of_the_restated_loss(ci, use_w):
    S, J, h, w = CASES[ci]
    p = ref.problem(S, J, h, w, CINS[ci], seed=1)
    r = ref.head_grad64(p.feat, p.w, p.b, p.target, p.tw, bool(use_w))
    loss, sse, dw, db = _autograd64(p, use_w)
    rel = [abs(r.loss - loss) / abs(loss), np.abs(r.sse - sse).max() / np.abs(sse).max(), np.abs(r.dw - dw).max() / np.abs(dw).max(),
           np.abs(r.db - db).max() / np.abs(db).max()]
    print("case %d use_w %d: loss, sse, dw, db relative to autograd %s" % (ci, use_w, ["%.2g" % v for v in rel]))
    assert max(rel) <= 1e-12
    import _val_ref
    o32 = r.o.reshape(S, J, h, w).astype(np.float32)            # the restated loss itself, on the fp32-rounded heat maps
    vm = _val_ref.val_metrics(o32, p.target, p.tw, bool(use_w))
    assert abs(vm.loss - r.loss) <= 1e-5 * r.loss


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_fp32_emulation_stays_inside_the_bound_and_three_defects_leave_it(ci):
    S, J, h, w = CASES[ci]
    p = ref.problem(S, J, h, w, CINS[ci], seed=2, nonzero=78 if CINS[ci] == 80 else None)
    assert ref.U == 2.0 ** -24
    for use_w in (True, False):
        r = ref.head_grad64(p.feat, p.w, p.b, p.target, p.tw, use_w)
        e = ref.excess(ref.emulate32(p.feat, p.w, p.b, p.target, p.tw, use_w), r)
        print("case %d use_w %d: emulation / bound (dw, db, loss, sse) %s" % (ci, use_w, ["%.3g" % v for v in e]))
        assert max(e) <= 1.0
        # the pixel whose loss would change one gradient element the most
        gf = np.abs(r.g).max(1) * np.abs(p.feat[..., :p.cin].reshape(S, h * w, p.cin)).max(2)
        drop = np.unravel_index(np.argmax(gf), gf.shape)
        for defect in ("drop", "tw", "bias"):
            if defect == "tw" and not use_w:
                continue
            d = ref.excess(ref.emulate32(p.feat, p.w, p.b, p.target, p.tw, use_w, defect=defect, drop=drop), r)
            print("case %d use_w %d: defect %-4s / bound (dw, db, loss, sse) %s" % (ci, use_w, defect, ["%.3g" % v for v in d]))
            assert max(d[0], d[1]) > 1.0, (defect, d)
            if defect == "bias":     # (a dropped or mis-weighted g leaves the loss alone: the loss is formed from o and tw, not from g)
                assert max(d[2], d[3]) > 1.0, (defect, d)
