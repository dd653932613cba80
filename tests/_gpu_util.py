"""Helpers for the -m gpu parity tests: NCHW CPU tensors <-> NHWC device activations of the engine."""
import torch

from i2r_amd import engine


def to_act(P, t, dt=0):
    """NCHW fp32 CPU tensor -> Act (NHWC, channels zero-padded to a multiple of 16; dt: 0 fp32 / 1 bf16 / 2 f16 storage) on P.device."""
    n, c, h, w = t.shape
    a = P.alloc(n, h, w, c, dt)
    buf = torch.zeros(n, h, w, a.cs)
    buf[..., :c] = t.permute(0, 2, 3, 1)
    a.view().copy_(buf.to(P.device))
    return a


def from_act(a):
    return a.view()[..., :a.c].permute(0, 3, 1, 2).contiguous().float().cpu()


def run(P):
    P.finalize()
    P.run()
    torch.cuda.synchronize()


# One 32-bit word that reads as NaN whatever the storage type of the buffer: fp32 0x7FC07FC0, and 0x7FC0 as bf16 and as f16.
NAN_WORD = 0x7FC07FC0


def tracked_program(device):
    """A Program that remembers every activation buffer it allocates (P.acts), for run_poisoned.  Program.alloc hands out torch.empty
    storage and recycles it by element count across shapes, so a kernel that leaves pad channels or tail rows unwritten is only caught on
    buffers that do not happen to hold zeros."""
    P = engine.Program(device)
    P.acts = []
    alloc = P.alloc

    def alloc_tracked(*args, **kw):
        a = alloc(*args, **kw)
        if all(a.t is not t for t in P.acts):
            P.acts.append(a.t)
        return a
    P.alloc = alloc_tracked
    return P


def run_poisoned(P, inputs, outputs, side_streams=None, hd=None):
    """Run a finished tracked_program twice and return the first run's output views (clones).

    Before the first run every activation buffer the program owns holds NaN, except the `inputs` (the Acts the test loaded through
    to_act).  After each run the whole extent n*h*w*cs of every output is finite and its pad channels [..., c:] are exactly 0.0; with
    hd (window attention: head pitch 40) the pad dims hd..39 of every head are 0.0 too.  The second run goes over the leftovers of the
    first -- only the inputs are loaded again, the emitters release them into the pool like any other buffer -- and must reproduce the
    first bit for bit."""
    P.finalize()
    saved = [a.t.clone() for a in inputs]
    own = {a.t.data_ptr() for a in inputs}
    assert all(any(a.t is t for t in P.acts) for a in list(inputs) + list(outputs)), "not a buffer of this tracked program"
    for t in P.acts:
        if t.data_ptr() not in own:
            t.view(torch.int32).fill_(NAN_WORD)
            assert torch.isnan(t).all()
    torch.cuda.synchronize()
    runs = []
    for rep in range(2):
        if rep:
            for a, s in zip(inputs, saved):
                a.t.copy_(s)
        P.run(side_streams)
        torch.cuda.synchronize()
        assert not P.sync_timed_out()
        got = [o.view().clone() for o in outputs]
        for o, g in zip(outputs, got):
            assert tuple(g.shape) == (o.n, o.h, o.w, o.cs)
            assert torch.isfinite(g.float()).all(), "run %d: non-finite values in an output (unwritten elements?)" % rep
            if o.cs > o.c:
                assert (g[..., o.c:] == 0).all(), "run %d: pad channels are not exactly zero" % rep
            if hd is not None and hd < 40:
                assert (g[..., :o.c].reshape(o.n, o.h, o.w, -1, 40)[..., hd:] == 0).all(), "run %d: pad dims of a head are not exactly zero" % rep
        runs.append(got)
    for a, b in zip(*runs):
        assert torch.equal(a, b), "the second run over the first one's leftovers differs"
    return runs[0]


def act_nchw(a, view):
    """the real channels of an output view of run_poisoned as an NCHW fp32 CPU tensor"""
    return view[..., :a.c].permute(0, 3, 1, 2).contiguous().float().cpu()
