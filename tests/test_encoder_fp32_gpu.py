"""-m gpu: every form of the fused fp32 encoder layer (enc_kv_k<5|6>, enc_layer4_k<DC, 12, QT, KS>) against float64 at ragged group
edges, through the raw C-ABI on poisoned buffers (tests/_encoder_cases.py: case table, references, harness).

Per layer the comparison is teacher-forced: the reference of layer i is the float64 oracle layer applied to the kernel's own stored output
of layer i-1, so errors do not compound and the fused K / V tail is judged on exactly what it consumed.  The bar is counted in units of
the fp32 CPU oracle's own error against float64 on that same input (E32): kernel max-abs <= 4 E32max (never above the 2e-4 of the older
tests), rms <= 3 E32rms.  Why a margin at all: the MFMA's 4-wide summation chains and the four-way key split reorder the sums, exp2 / rcp /
rsqrt are ~1 ulp hardware approximations, and the max over ~1e5 outputs sits on a few ill-conditioned tokens.  The measured ratios per case
are tabled in DESIGN.md ("fp32 encoder kernels against float64")."""
import ctypes as C

import pytest
import torch

import _encoder_cases as ec
from _gpu_util import run
from i2r_amd import cabi, engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_FACTOR, RMS_FACTOR, MAX_CAP, STACK_BAR = 4.0, 3.0, 2e-4, 3e-4


def _stack(name, d, nl):
    case = ec.CASES[name]
    src, pos, table, mode = ec.inputs(name, d, nl)
    st = ec.Stack(case.lens, d, nl, DEV, src, None if table is not None else pos, table, case.scratch, case.tail)
    return st, src, pos, mode


def _judge(tag, got, ref64, ref32, cap=None):
    """the 4 x / 3 x rule; prints the measured ratios before it asserts"""
    e_max, e_rms = ec.err_max_rms(ref32, ref64)
    k_max, k_rms = ec.err_max_rms(got, ref64)
    print("ENC-RATIO %s max %.3e / %.3e = %.2f rms %.3e / %.3e = %.2f" % (tag, k_max, e_max, k_max / e_max, k_rms, e_rms, k_rms / e_rms))
    bar = MAX_FACTOR * e_max if cap is None else min(MAX_FACTOR * e_max, cap)
    assert k_max <= bar, "%s: max-abs %.3e above %.3e (fp32 oracle %.3e)" % (tag, k_max, bar, e_max)
    assert k_rms <= RMS_FACTOR * e_rms, "%s: rms %.3e above %g x %.3e" % (tag, k_rms, RMS_FACTOR, e_rms)


def _check_kv(tag, st, kbuf, vbuf, i, x_in, pos):
    """the fragment-packed K / V^T images of layer i against the float64 projections of its input"""
    frag, row, n_frag = ec.key_slots(st.lens)
    K, V = ec.unpack_kv(kbuf, n_frag, st.cs), ec.unpack_kv(vbuf, n_frag, st.cs, vt=True)
    valid = torch.zeros(n_frag, 16, dtype=torch.bool)
    valid[frag, row] = True
    assert torch.isfinite(K).all(), tag + ": K not finite (a key past a group's end included)"
    assert (V[~valid] == 0.0).all(), tag + ": V at keys past a group's end is not exactly 0.0"
    k64, v64 = ec.ref_kv(st.d, i, x_in, pos, st.n_cov)
    k32, v32 = ec.ref_kv(st.d, i, x_in, pos, st.n_cov, torch.float32)
    _judge(tag + " K", K[frag, row, :st.d], k64, k32)
    _judge(tag + " V", V[frag, row, :st.d], v64, v32)
    if st.cs > st.d:
        assert (K[frag, row, st.d:] == 0.0).all() and (V[frag, row, st.d:] == 0.0).all()


def _check_run(tag, st, r, src, pos):
    n, d, nl = st.n_cov, st.d, st.n_layers
    qt, ks, grid = st.form
    # ---- nothing else written ----
    for s, snap in enumerate(r.snaps):
        if snap["cnt"] is not None:
            assert (snap["cnt"] == 0).all(), "%s: split_cnt not zero behind launch %d" % (tag, s)
        for b in snap["k"] + snap["v"]:
            assert ec.is_poison(b[st.kv_used:]), "%s: K / V workspace written past fragment n_qtiles16 (launch %d)" % (tag, s)
    if r.snaps[-1]["ws"] is not None and ks == 1:
        assert ec.is_poison(r.snaps[-1]["ws"]), tag + ": split_ws touched by a form without a key split"
    for i, o in enumerate(r.outs):
        assert torch.isfinite(o[:n]).all(), "%s: layer %d output not finite over the group rows" % (tag, i)
        assert ec.is_poison(o[n:]), "%s: layer %d wrote rows past the last group offset" % (tag, i)
        if st.cs > d:
            assert (o[:n, d:] == 0.0).all(), "%s: layer %d pad columns not exactly zero" % (tag, i)
    # ---- K / V images: of layer 0 behind the kv launch, of layer i + 1 behind layer i's fused tail ----
    _check_kv(tag + " kv0", st, r.snaps[0]["k"][0], r.snaps[0]["v"][0], 0, src, pos)
    for i in range(nl - 1):
        _check_kv(tag + " kv%d" % (i + 1), st, r.snaps[i + 1]["k"][(i + 1) % 2], r.snaps[i + 1]["v"][(i + 1) % 2], i + 1, r.outs[i][:, :d], pos)
    if nl == 1:   # no fused tail: the other pair stays untouched
        assert ec.is_poison(r.snaps[-1]["k"][1]) and ec.is_poison(r.snaps[-1]["v"][1])
    # ---- per layer, teacher-forced ----
    for i in range(nl):
        x_in = src if i == 0 else r.outs[i - 1][:, :d]
        _judge("%s layer%d" % (tag, i), r.outs[i][:n, :d], ec.ref_layer(d, i, x_in, pos, st.lens), ec.ref_layer(d, i, x_in, pos, st.lens, torch.float32),
               cap=MAX_CAP)
    if nl > 1:
        err = (r.outs[-1][:n, :d].double() - ec.ref_stack(d, nl, src, pos, st.lens)[-1]).abs().max().item()
        print("ENC-STACK %s end-to-end max-abs %.3e" % (tag, err))
        assert err <= STACK_BAR, "%s: %d-layer stack max-abs %.3e" % (tag, nl, err)


def _same_run(a, b):
    """every layer output and the K / V pair each launch wrote (launch 0 = kv: pair 0; layer i with a fused tail: pair (i + 1) % 2), bit
    for bit.  (The pair a launch did not write holds poison in a first run and leftovers in a replay.)"""
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    wrote = [(s, s % 2) for s in range(len(a.outs))]
    return all(same(x, y) for x, y in zip(a.outs, b.outs)) and all(
        same(a.snaps[s][kv][p], b.snaps[s][kv][p]) for s, p in wrote for kv in ("k", "v"))


@pytest.mark.parametrize("name,d,nl", ec.VARIANTS, ids=["%s-d%d-L%d" % v for v in ec.VARIANTS])
def test_case_against_float64_on_poisoned_buffers(name, d, nl):
    st, src, pos, mode = _stack(name, d, nl)
    tag = "%s d%d L%d pos-%s %s%s" % (name, d, nl, mode, ec.FORM_NAMES[st.form[:2]], st.form)
    print("ENC-FORM %s" % tag)
    r = st.run()
    _check_run(tag, st, r, src, pos)
    # replay over the first run's leftovers, only src poisoned and loaded again: bit-identical, counters still zero
    st.load_src()
    r2 = st.run(poison=False)
    assert _same_run(r, r2), tag + ": the replay differs"
    assert all(s["cnt"] is None or (s["cnt"] == 0).all() for s in r2.snaps)


@pytest.mark.parametrize("name", ["one-edge", "split-edge", "two-edge"])
@pytest.mark.parametrize("d", ec.DIMS)
def test_groups_are_independent_bit_for_bit(name, d):
    """other tokens in every third group: output rows and K / V fragments of all other groups do not change by a bit, those of the changed
    groups do"""
    st, src, pos, _ = _stack(name, d, 3)
    a = st.run()
    offs = ec.offsets(st.lens)
    changed = [g for g in range(len(st.lens)) if g % 3 == 1]
    src2 = src.clone()
    for g in changed:
        src2[offs[g]:offs[g + 1]] = ec._rand((st.lens[g], d), "other%s%d_%d" % (name, d, g), 1.3)
    st.load_src(src2)
    b = st.run()
    row_changed = torch.zeros(st.rows, dtype=torch.bool)
    frag_changed = torch.zeros(ec.counts(st.lens)[0], dtype=torch.bool)
    base = 0
    for g, n in enumerate(st.lens):
        if g in changed:
            row_changed[offs[g]:offs[g + 1]] = True
            frag_changed[base:base + -(-n // 16)] = True
        base += -(-n // 16)
    bits = lambda t: t.contiguous().view(torch.int32)
    for i, (x, y) in enumerate(zip(a.outs, b.outs)):
        assert torch.equal(bits(x[~row_changed]), bits(y[~row_changed])), "layer %d: rows of an unchanged group moved" % i
        assert all((x[offs[g]:offs[g + 1]] != y[offs[g]:offs[g + 1]]).any() for g in changed), "layer %d: a changed group did not change" % i
    n_frag = frag_changed.numel()
    for s, (sa, sb) in enumerate(zip(a.snaps, b.snaps)):
        for x, y in zip(sa["k"] + sa["v"], sb["k"] + sb["v"]):
            if ec.is_poison(x[:st.kv_used]):
                assert ec.is_poison(y[:st.kv_used])   # (the second pair before the first fused tail)
                continue
            fx, fy = x[:st.kv_used].view(n_frag, -1), y[:st.kv_used].view(n_frag, -1)
            assert torch.equal(bits(fx[~frag_changed]), bits(fy[~frag_changed])), "launch %d: K / V fragments of an unchanged group moved" % s
            assert ((fx != fy).any(1) == frag_changed).all(), "launch %d: a fragment of a changed group did not change" % s


@pytest.mark.parametrize("d", ec.DIMS)
def test_one_program_regrouped_across_the_forms_equals_the_harness(d):
    """Program.encoder(regroupable=True) + set_groups in the sequence one-edge -> split-edge -> two-edge -> one-edge over one token buffer,
    the program's K / V workspaces poisoned before each step: every step equals the harness for that grouping bit for bit"""
    seq = ["one-edge", "split-edge", "two-edge", "one-edge"]
    crops, per = 724, 17                                   # 12308 tokens = the tokens of two-edge; room for one group per crop
    rows = crops * per
    assert rows == sum(ec.CASES["two-edge"].lens)
    cs = (d + 15) // 16 * 16
    src, posr = ec._rand((rows, d), "rgsrc%d" % d), ec._rand((rows, d), "rgpos%d" % d, 0.5)
    dev = torch.device(DEV)
    P = engine.Program(dev)
    fa, pa = P.alloc(crops, per, 1, d), P.alloc(crops, per, 1, d)
    for a, t in ((fa, src), (pa, posr)):
        buf = torch.zeros(rows, cs)
        buf[:, :d] = t
        a.view().copy_(buf.view(crops, per, 1, cs).to(dev))
    layers = ec.packed_layers(d, 3, DEV)
    out = P.encoder(fa, layers, ec.offsets(ec.CASES[seq[0]].lens), pos=pa.ptr, regroupable=True)
    grouping, tok = P.groupings[-1]
    assert tok == per
    ptrs = {p for desc, _ in grouping["descs"] for p in (desc.kbuf, desc.vbuf)}
    work = [t for t in P.keep if isinstance(t, torch.Tensor) and t.data_ptr() in ptrs]
    assert len(work) == 4 == len(ptrs)
    forms, first = [], None
    for name in seq:
        lens = ec.CASES[name].lens
        n = sum(lens)
        P.set_groups(grouping, ec.offsets(lens))
        forms.append(ec.layer_form(grouping["descs"][0][0])[:2])
        for t in work:
            t.view(torch.int32).fill_(ec.NAN_WORD)
        run(P)
        got = out.view().reshape(rows, cs)[:n].cpu()
        want = ec.Stack(lens, d, 3, DEV, src[:n], posr[:n]).run().outs[-1]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name
        first = got if first is None else first
    assert torch.equal(got.view(torch.int32), first.view(torch.int32))
    assert forms == [(1, 1), (1, 2), (2, 1), (1, 1)]


@pytest.mark.parametrize("d", ec.DIMS)
def test_bad_descriptors_are_rejected_and_nothing_is_written(d):
    st, _, _, _ = _stack("one-edge", d, 3)
    L, stream = cabi.lib(), torch.cuda.current_stream().cuda_stream
    ok = st.descs[0]
    for bad in (dict(cs=64), dict(dff_pad=96), dict(out=ok.src), dict(next_kbuf=ok.kbuf), dict(n_qtiles16=0), dict(w1=None)):
        desc = cabi.EncoderDesc()
        C.memmove(C.byref(desc), C.byref(ok), C.sizeof(desc))
        for k, v in bad.items():
            setattr(desc, k, v)
        st.poison()
        st.load_src()
        assert L.i2r_encoder_kv(C.byref(desc), stream) != 0 and b"i2r_encoder" in L.i2r_last_error(), bad
        assert L.i2r_encoder_layer(C.byref(desc), stream) != 0 and b"i2r_encoder" in L.i2r_last_error(), bad
        torch.cuda.synchronize()
        assert all(ec.is_poison(t.cpu()) for t in st.workspaces()), bad
        assert (st.split_cnt == ec.CNT_POISON).all() and torch.equal(st.src.cpu(), st.src_host), bad
