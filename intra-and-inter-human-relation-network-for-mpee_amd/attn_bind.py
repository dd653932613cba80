"""The work of an attention-map capture behind the program's head (attn_capture.Form.behind), per kind one pair: bind(P, plans, glens, buf,
rows, held, call), the tail of Program.bind_capture, makes the call's record Capture.call of every capture of program P; run(P, multi, S, H)
issues the work on the current stream behind the program's run, on the q|k the captured layers kept -> what the form's result() needs of it.
Nothing here reads the device."""
import ctypes as C

import torch

from . import attn_capture, cabi


def _joint_tokens(P, multi, S, H):
    """the tables of a joint-form program: i2r_joint_tokens on the (merged) heat maps multi [S, J, H/4, W/4] fills the token tables
    bind_capture made; the launches that read them follow.  -> (joints [S, J, 2], maxvals [S, J]) on the device"""
    assert multi.is_contiguous() and multi.shape[0] == S and 1 <= len(P.captures) <= cabi.MAX_TOKEN_TABLES
    J, hh, hw = multi.shape[1:]
    joints = torch.empty(S, J, 2, dtype=torch.float32, device=P.device)
    maxvals = torch.empty(S, J, dtype=torch.float32, device=P.device)
    a = cabi.JointTokensArgs(heatmaps=multi.data_ptr(), points=joints.data_ptr(), maxvals=maxvals.data_ptr(), n_crops=S, joints=J, hh=hh, hw=hw,
                             in_stride=H // hh, n_tables=len(P.captures))
    for t, cap in zip(a.table, P.captures):
        tok, _, crops = cap.tables
        assert crops.shape == (2, S)
        t.tokens, t.crop_group, t.crop_slot = tok.data_ptr(), crops[0].data_ptr(), crops[1].data_ptr()
        (t.n_grp, t.K), t.fh, t.fw, t.down = tok.shape, cap.x.h, cap.x.w, H // cap.x.h
    cabi.check(cabi.lib().i2r_joint_tokens(C.byref(a), torch.cuda.current_stream(P.device).cuda_stream), "i2r_joint_tokens")
    return joints, maxvals


def run_launches(P, multi, S, H):
    """the plain joint form: i2r_joint_tokens, then the launch of every captured layer"""
    jt = _joint_tokens(P, multi, S, H)
    launch, stream = getattr(cabi.lib(), P.form.entry), torch.cuda.current_stream(P.device).cuda_stream
    for cap in P.captures:
        for _, a in cap.ops:
            cabi.check(launch(C.byref(a), stream), P.form.entry)
    return jt


def _aim(a, fields, *values):
    for f, v in zip(fields, values):
        if f:
            setattr(a, f, v)
    return a


def bind_merge(P, plans, glens, buf, rows, held, call):
    """a merged form (attn_capture.Form.merge): per capture a Merge -- per captured layer the launch args of either half of the flip
    program (the mirrored groups repeat the plain ones half the stack's rows further on, so ONE offset table serves both: the mirrored
    half's args are a copy of the plain half's aimed at its own q|k rows, token table and workspaces) and the i2r_attn_flip_merge args,
    whose out is the layer's maps block in buf; the two raw workspaces are shared by all layers (the launches are ordered on the stream)."""
    form, base = P.form, 0
    raw = [torch.empty(max(p.raw_floats for p in plans), dtype=torch.float32, device=P.device) for _ in range(2)]
    held += raw
    for cap, lens, p in zip(P.captures, glens, plans):
        cur, n = cap.grouping["current"], len(lens)
        half = (len(cur) - 1) // 2
        assert len(cur) == 2 * half + 1 and n <= half and all(cur[half + g] - cur[half] == cur[g] for g in range(n + 1)), "not a flip program's groups"
        tok = (cap.tables[0], torch.empty_like(cap.tables[0])) if cap.tables else (None, None)
        rel = [torch.empty(p.blocks[0].offs[-1], dtype=torch.float32, device=P.device) for _ in range(2)] if form.HALF[4] else None
        m = cap.call = attn_capture.Merge(tok, rel)
        raw_off = torch.tensor(p.raw_offs, dtype=torch.int64).pin_memory().to(P.device, non_blocking=True) if p.raw_floats else None
        held += [m, raw_off]
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        for _, a in cap.ops:
            _aim(a, form.HALF, a.qk, ptr(tok[0]), raw[0].data_ptr(), ptr(raw_off), ptr(rel and rel[0]))
            b = _aim(type(a).from_buffer_copy(a), form.HALF, a.qk + 4 * cur[half] * a.qk_cs, ptr(tok[1]), raw[1].data_ptr(), ptr(raw_off), ptr(rel and rel[1]))
            fm = p.raw_floats and cabi.AttnFlipMergeArgs(  # (out: the layer's last set, the per-person form's behind the relation blocks)
                a=raw[0].data_ptr(), b=raw[1].data_ptr(), out=buf.data_ptr() + 4 * (base + p.blocks[-1].base), grp_off=a.grp_off, src_off=raw_off.data_ptr(),
                out_off=cap.off[-1].data_ptr(), q_cnt=0 if rel else cap.tables[1].data_ptr(), grp_off_host=a.grp_off_host,
                n_grp=n, K=p.K, seg=a.seg if rel else 0, scale=form.scales[cap.stack], h=cap.x.h, w=cap.x.w)
            m.layers.append((a, b, fm, rel and buf[base:base + p.blocks[0].offs[-1]]))
            base += p.layer_floats


def run_merge(P, multi, S, H):
    """a merged form: (the joint form: i2r_joint_tokens;) i2r_token_mirror makes the mirrored pass's token table, then per captured layer
    the form's launch at scale 1 on either half and ONE i2r_attn_flip_merge into the capture buffer; the relation matrices of the per-person
    form, mirror-invariant sums over whole persons, are merged by one torch expression on the same stream: R_m = (R + R') / 2."""
    L, stream, form = cabi.lib(), torch.cuda.current_stream(P.device).cuda_stream, P.form
    jt, launch = _joint_tokens(P, multi, S, H) if form.J else None, getattr(L, form.entry)
    for cap in P.captures:
        m = cap.call
        if m.tok[0] is not None:
            cabi.check(L.i2r_token_mirror(m.tok[0].data_ptr(), m.tok[1].data_ptr(), m.tok[0].numel(), cap.x.w, stream), "i2r_token_mirror")
        for a, b, fm, rel_out in m.layers:
            cabi.check(launch(C.byref(a), stream), form.entry)
            cabi.check(launch(C.byref(b), stream), form.entry)
            if fm:
                cabi.check(L.i2r_attn_flip_merge(C.byref(fm), stream), "i2r_attn_flip_merge")
            if m.rel:
                torch.add(m.rel[0], m.rel[1], out=rel_out).mul_(0.5)
    return jt


def bind_rollout(P, plans, glens, buf, rows, held, call):
    """the roll-out form (attn_capture.RolloutForm): per capture a Chain -- the seed of the chain (flat indices into the first working
    matrix, uploaded here), the steps in chain order (side 0: layers hi -> lo, side 1: lo -> hi), each reading the matrix the step
    before wrote, the last one writing (and up-sampling) into the stack's blocks, and for the per-person form the views the [P, P]
    relations are reduced from and into.  call.alpha: this call's (the program is not keyed by it)."""
    form = P.form
    for cap, lens, p in zip(P.captures, glens, plans):
        xl, res = p.blocks[-1], p.blocks[-2]  # the working matrices' layout; the set the last step writes (maps)
        x0, n_x = cap.base + xl.base, p.extra_floats // 2
        X = [buf[x0:x0 + n_x], buf[x0 + n_x:x0 + 2 * n_x]]
        seed = p.seed[0].pin_memory().to(P.device, non_blocking=True)
        scale = form.scales[cap.stack]
        ops = sorted(cap.ops, key=lambda o: o[0], reverse=form.side == 0)
        to_blocks = res.shapes is not None  # (per person without maps: the chain ends in a working matrix)
        for n, (_, a) in enumerate(ops):
            a.in_, a.out, a.x_off, a.out_off, a.scale, a.alpha = X[n % 2].data_ptr(), X[(n + 1) % 2].data_ptr(), cap.off[-1].data_ptr(), None, 1, call.alpha
        if to_blocks:  # (the last step)
            a.out, a.out_off, a.scale = buf.data_ptr() + 4 * (cap.base + res.base), cap.off[-2].data_ptr(), scale
        r = cap.call = attn_capture.Chain(X[0], seed, p.seed[1], [a for _, a in ops], None)
        if not form.points:  # R_T from the raw rows of the last step: in the maps blocks at scale 1, else in the working matrix / rows
            cur = cap.grouping["current"]
            if to_blocks and scale > 1:
                raw = [rows[p.K * cur[g]:p.K * cur[g] + (n // a.seg) * n] for g, n in enumerate(lens)]
            else:
                src, b0 = (buf, cap.base + res.base) if to_blocks else (X[len(ops) % 2], 0)
                raw = [src[b0 + o:b0 + e] for o, e in zip(xl.offs, xl.offs[1:])]
            rb = cap.base + p.blocks[0].base
            r.rel = [(v.view(n // a.seg, n // a.seg, a.seg), buf[rb + o:rb + e].view(n // a.seg, n // a.seg))
                     for v, n, o, e in zip(raw, lens, p.blocks[0].offs, p.blocks[0].offs[1:])]
        held += [seed, r]


def run_rollout(P, multi, S, H):
    """the roll-out form: the seed by two torch fills, the chain of i2r_attn_rollout_step launches, and for the per-person form
    R_T = sum_{k in j} D_T = mean_{q in i} F_T as one torch reduction per image"""
    L, stream = cabi.lib(), torch.cuda.current_stream(P.device).cuda_stream
    for cap in P.captures:
        r = cap.call
        r.X0.zero_().index_fill_(0, r.seed, r.value)
        for a in r.steps:
            cabi.check(L.i2r_attn_rollout_step(C.byref(a), stream), "i2r_attn_rollout_step")
        for rows, rel in r.rel or ():
            if P.form.side == 0:
                torch.sum(rows, 2, out=rel)
            else:
                rel.copy_(rows.mean(2).t())


# (the plain joint form binds nothing of its own: bind_capture patched its launches and made the tables the device fills)
PAIRS = {"launches": (lambda *call: None, run_launches), "merge": (bind_merge, run_merge), "rollout": (bind_rollout, run_rollout)}
