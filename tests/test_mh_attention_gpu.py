"""-m gpu: every instantiation of the multi-head attention kernel (enc_mh_attn_k<HB, NQ>, 24 of them) against float64 at ragged group
edges, through the raw C-ABI on poisoned buffers (tests/_mh_cases.py: case table, inputs, reference, harness; tests/test_mh_cases.py: what
the table reaches and why the tolerance is not what makes a case pass).

Each case is one launch: max |got - float64| < 2e-5 (the project's bar for this operation at |v| <= 1, test_kernels_gpu.py), the pad dims of
every head and the columns behind the heads exactly 0, guard and tail rows still the poison word, no NaN in a group row (the stride gaps,
the tail rows and -- under key_len -- the k and v parts of every non-key row are NaN on the device), and a second launch into a re-poisoned
buffer bit-identical.

Measured on an MI355X, worst err / 2e-5 per instantiation over the cases that run it (MH-RATIO lines of this module):

    HB   NQ = 1                NQ = 2                NQ = 4
    1    0.023 w16-h1          0.045 n2-w16          0.105 rise-n4
    2    0.064 kl-clamp        0.162 rise-n2         0.077 n4-w32
    3    0.188 rise-n1         0.092 t2-4096-w48
    4    0.088 w64-h4          0.113 st-n2
    5    0.090 w80-h8          0.122 kl-n2
    6    0.132 t2-4095         0.146 t2-4096
    7    0.148 far-w112
    8    0.136 w128-h7
    9    0.094 w144-h1
    10   0.132 w160-h2
    11   0.115 w176-h3
    12   0.161 w192-h4
    13   0.145 w208-h8
    14   0.193 w224-h5
    15   0.135 w240-h6
    16   0.137 w256-h7

(the case named is the one with that worst ratio).  Worst of all: 0.193 (w224-h5); the rising cases at scale 6 are the largest of their
widths, as their fp32 restatements on the CPU are.  No kernel or launcher bug was found.  The wide heads (HB >= 12, up to 214 VGPRs,
profiles/attn_maps_core_resources.md) are not slow at these sizes: no case takes a second, float64 reference included, and the module
runs in 13 s."""
import pytest
import torch

import _mh_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(mc.CASES))
def test_case_against_float64_on_poisoned_buffers(name):
    case = mc.CASES[name]
    run = mc.Launch(name, DEV)
    f = run.form
    assert (f.hb, f.nq) == (case.hp // 16, case.nq), "the case is there for <%d,%d>" % (case.hp // 16, case.nq)
    hs, _, _, _, out_cs = mc.strides(case)
    n, G = run.n_tok, mc.GUARD_ROWS
    whole = run.run()
    rows = whole[G:G + n]
    # ---- nothing else written, nothing forbidden read ----
    assert mc.is_poison(whole[:G]) and mc.is_poison(whole[G + n:]), name + ": guard or tail rows written"
    assert not torch.isnan(rows).any(), name + ": NaN in a group row (unwritten, or a row or column outside the group's keys was read)"
    got = rows[:, :hs].reshape(n, case.heads, case.hp)
    assert (got[..., case.hd:] == 0.0).all(), name + ": pad dims of a head not exactly 0"
    assert (rows[:, hs:] == 0.0).all(), name + ": columns behind the heads not exactly 0"
    # ---- the values ----
    err = (got[..., :case.hd].double() - mc.reference(name)).abs().max().item()
    print("MH-RATIO <%d,%d> %-12s grid %s x %d err %.3e = %.3f TOL" % (f.hb, f.nq, name, f.grid, f.block, err, err / mc.TOL))
    assert err < mc.TOL, "%s <%d,%d>: max-abs %.3e" % (name, f.hb, f.nq, err)
    # ---- fixed order, no atomics ----
    again = run.run()
    assert torch.equal(whole.view(torch.int32), again.view(torch.int32)), name + ": the second launch differs"
