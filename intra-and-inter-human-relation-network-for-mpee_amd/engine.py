"""Execution engine of the hot path: replays a pre-built launch program through the C-ABI (cabi.py) over the weights that pack.py
laid out for the HIP kernels.  No arithmetic happens in Python/torch here: torch only owns device memory and streams.

A Program is the static list of launches for one (S, H, W, length) signature: all intermediate NHWC buffers
are pre-allocated (arena with reuse), so a forward is ONE call into i2r_run_program.
"""
import ctypes as C
import math
import os

import torch

from . import attn_bind, attn_capture, cabi
from .attn_capture import AttnQueries, JointQueries, PersonMaps, Rollout, TargetMaps  # noqa: F401 (the capture forms' public classes stay importable from here)
from .pack import (PRECISIONS, PackedConv, Packer, _m16, _r16, fold_bn, pack_frag, pack_frag32, pack_k4, pack_k8,  # noqa: F401 (the packing names stay importable from here)
                   winograd_weights)


def wino_fragment(conv_h, conv_w):
    """(fragment width, height) in output pixels of the Winograd kernels for a map: 16 tiles as 8x2, 4x4 or 2x8 -- the shape that
    covers the map with the fewest fragments (same rule as prepare_wino in csrc/i2r_conv_plan.h)"""
    best = None
    for fw in (8, 4, 2):
        n = -(-conv_w // (2 * fw)) * -(-conv_h // (32 // fw))
        if best is None or n < best[0]:
            best = (n, 2 * fw, 32 // fw)
    return best[1], best[2]


LP1X1 = True  # 16-bit modes: single 1x1 convs over few pixels on i2r_conv1x1_lp
# ... up to this many pixels per batch: beyond that the implicit-GEMM kernel has enough workgroups to hide its staging.  The kernel is
# chosen by the batch's pixel count, so a crop's 16-bit heat map is tolerance-stable, not bit-stable, across batch sizes (fp32 results do
# not depend on the batch).
LP1X1_MAX_PIX = 65536
# branch widths whose transformer-block halves run as the fused 16-bit kernels (i2r_hrt_attn_block / i2r_hrt_mlp_block)
_HRT_FUSED_ATTN = (78, 156, 312)
_HRT_FUSED_MLP = (78, 156, 312)
_MLP_VARIANT = {78: 1, 156: 2, 312: 2}  # measured (tools/time_hrt_mlp.py, host_rate.py): C = 156 29.0 -> 22.0 us, config 5 forward 4.19 -> 3.87 ms
PAIR1X1 = True  # layer1's conv3 + next conv1 as one i2r_conv1x1_pair launch (fp32)
FUSE_IN = True  # the closing pass of an HRNet fuse layer rides in the staging of the next module's first Winograd conv (fp32)
PRUNE_FUSE = True  # the last HRNet module computes only the fuse outputs its caller reads (HRNetW48.emit(need=...))
WINOGRAD = True  # fp32 3x3 stride-1 convs on the Winograd F(2x2, 3x3) kernels
WINO_SEQ = True  # ... whose workgroups run several fragments on one set-up, as many as the library chooses per launch (i2r_conv_desc.seq = 0; False: one)
WINO_FORMS = True  # ... with the epilogue compiled per shape (bias + ReLU, bias + res1 + ReLU; i2r_conv_wino_forms); False: the general epilogue, same bits
CONV_FORMS = True  # direct fp32 convs (conv_igemm_f32) on their single-chunk / pipelined bodies and epilogue forms (i2r_conv_direct_forms); False: the general body, same bits
# fork / join / record / wait as device-side signal / wait kernels (csrc/i2r_api.hip) when the lanes are independent queues.  A wait kernel
# spins until ANOTHER kernel signals it: under a tool that lets one kernel run at a time (rocprofv3 counter collection serialises dispatches)
# it could only time out, so the event form is used whenever a profiler library is attached to the process.
PROFILER_ATTACHED = bool(os.environ.get("ROCP_TOOL_LIBRARIES") or os.environ.get("ROCPROFILER_LIBRARY_CTOR") or os.environ.get("HSA_TOOLS_LIB")
                         or any(t in os.environ.get("LD_PRELOAD", "") for t in ("rocprof", "roctracer", "rocprofiler")))  # rocprofv3 / rocprofv2 / rocprof / preloaded tools
DEVICE_SYNC = not PROFILER_ATTACHED


# ------------------------------------------------------------------------------------------------
# program
# ------------------------------------------------------------------------------------------------
class Act:
    """NHWC activation buffer [n, h, w, cs] holding c real channels; dt = storage type: 0 fp32, 1 bf16, 2 f16 (the conv towers of
    the 16-bit modes keep their maps in 16 bit; `t` is the raw storage as a float32 tensor of numel * (4 or 2) / 4 words)."""
    __slots__ = ("t", "n", "h", "w", "c", "cs", "dt")
    TORCH_DT = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}

    def __init__(self, t, n, h, w, c, cs, dt=0):
        self.t, self.n, self.h, self.w, self.c, self.cs, self.dt = t, n, h, w, c, cs, dt

    def view(self):
        """[n, h, w, cs] tensor view of the storage in its own dtype"""
        return self.t.view(self.TORCH_DT[self.dt])[:self.n * self.h * self.w * self.cs].view(self.n, self.h, self.w, self.cs)

    @property
    def ptr(self):
        return self.t.data_ptr()


class _RawAct:
    """a device buffer laid out like the Act `like` (of n crops, if given) that the program does not own: a conv's second input, the
    source of a gather segment bound per call"""
    __slots__ = ("ptr", "n", "h", "w", "c", "cs", "dt")

    def __init__(self, ptr, like, n=None):
        self.ptr, self.n, self.h, self.w, self.c, self.cs, self.dt = ptr, like.n if n is None else n, like.h, like.w, like.c, like.cs, 0


_MT_EFF = {1: 0.62, 2: 0.9, 3: 1.0, 4: 0.9}  # measured on MI355X (tools/sweep_conv.py): B-fragment reuse per wave


def choose_tile(conv_h, conv_w, wm, stride, max_d, n_img, n_cblk, force_mt=0, want_cost=False):
    """(tile_h, tile_w, mt) for a workgroup of wm M-waves.  Cost model fitted to tools/sweep_conv.py on MI355X:
    time ~ rounds of 256 workgroups x padded pixels per workgroup / per-wave efficiency(mt), plus a halo-staging term."""
    best = None
    cands_w = sorted({w for w in (conv_w, 48, 32, 24, 16, 12, 8, 6, 4) if w <= conv_w and w <= 48})
    for mt in ((force_mt,) if force_mt else (1, 2, 3, 4)):
        cap = wm * mt * 16
        for tw in cands_w:
            th = min(conv_h, cap // tw)
            if th < 1:
                continue
            ph, pw = (th - 1) * stride + max_d + 1, (tw - 1) * stride + max_d + 1
            if ph * pw > 1280:
                continue
            tiles = -(-conv_h // th) * -(-conv_w // tw)
            blocks = tiles * n_img * n_cblk
            rounds = -(-blocks // 256)
            halo = ph * pw / float(th * stride * tw * stride)
            cost = rounds * (cap / _MT_EFF[mt]) * (1.0 + 0.08 * (halo - 1.0))
            if best is None or cost < best[0] - 1e-9:
                best = (cost, th, tw, mt)
    assert best is not None, "no tile for %dx%d" % (conv_h, conv_w)
    if want_cost:
        return best
    return best[1], best[2], best[3]


_LPT_CACHE = {}  # (counts, works, n_cu) -> dispatch order (a stage's modules repeat the same signature; a table costs ~25 ms of Python)
_LPT_DEV = {}    # (device, counts, works) -> the table as a device tensor, shared by every program of the device


def lpt_block_table(device, counts, works):
    """device int32 tensor of lpt_block_order(counts, works), built once per signature and device"""
    key = (str(device), tuple(counts), tuple(works))
    t = _LPT_DEV.get(key)
    if t is None:
        ck = (tuple(counts), tuple(works), 256)
        if ck not in _LPT_CACHE:
            _LPT_CACHE[ck] = lpt_block_order(counts, works)
        t = _LPT_DEV[key] = torch.tensor(_LPT_CACHE[ck], dtype=torch.int32, device=device)
    return t


def lpt_block_order(counts, works, n_cu=256):
    """Dispatch order for a grouped launch whose members have different per-workgroup work (K): longest-processing-
    time packing of all workgroups onto n_cu bins, emitted round by round (bin0[r], bin1[r], ...), so the first n_cu
    workgroups (one per CU) are the heaviest and every CU ends up with about the same total. Entry = member << 24 | idx."""
    import heapq
    items = sorted(((w, g, i) for g, (c, w) in enumerate(zip(counts, works)) for i in range(c)),
                   key=lambda t: (-t[0], t[1], t[2]))
    heap = [(0, b) for b in range(n_cu)]
    bins = [[] for _ in range(n_cu)]
    for w, g, i in items:
        load, b = heapq.heappop(heap)
        bins[b].append((g << 24) | i)
        heapq.heappush(heap, (load + w, b))
    out, r = [], 0
    while len(out) < len(items):
        for b in range(n_cu):
            if r < len(bins[b]):
                out.append(bins[b][r])
        r += 1
    return out


def conv_split(cout_pad):
    nfrag = cout_pad // 16
    nt = next(c for c in (3, 4, 5) if nfrag % c == 0)  # same rule as csrc/i2r_conv_plan.h
    nb = nfrag // nt
    wn = 4 if nb % 4 == 0 else 2 if nb % 2 == 0 else 1
    return nt, wn


_wino_forms_pushed = None


def push_wino_forms():
    """WINO_FORMS -> the library's process-wide switch (i2r_conv_wino_forms), where a launch resolves its form; called where Winograd
    descriptors are made and before a program runs, one comparison when nothing changed"""
    global _wino_forms_pushed
    if _wino_forms_pushed != bool(WINO_FORMS):
        cabi.check(cabi.lib().i2r_conv_wino_forms(int(bool(WINO_FORMS))), "i2r_conv_wino_forms")
        _wino_forms_pushed = bool(WINO_FORMS)


_conv_forms_pushed = None


def push_conv_forms():
    """CONV_FORMS -> the library's process-wide switch (i2r_conv_direct_forms); a launch resolves its form when it runs, so this is
    called before a program runs, one comparison when nothing changed"""
    global _conv_forms_pushed
    if _conv_forms_pushed != bool(CONV_FORMS):
        cabi.check(cabi.lib().i2r_conv_direct_forms(int(bool(CONV_FORMS))), "i2r_conv_direct_forms")
        _conv_forms_pushed = bool(CONV_FORMS)


class Program:
    def __init__(self, device):
        self.device = device
        self.ops = []        # (kind, lane, struct)
        self.keep = []       # everything the structs point to
        self.pool = {}       # numel -> [tensor]
        self.pending = []    # buffers released inside a fork region: reusable only after the join
        self.lane_pool = {}  # (lane, numel) -> buffers released by that lane inside the current fork region
        self.lane_ctx = 0    # lane whose ops are being emitted (set by the emitters inside a fork region)
        self.groupings = []  # (grouping, tokens per crop) of encoders whose groups follow `length` (set_groups)
        self.enc_stacks = []
        self.split_counters = []  # hand-off counters of the encoder stacks (zero between launches; re-zeroed when a run fails)
        self.captures = []   # encoder stacks whose attention maps this program computes (_capture_begin)
        self.form = None     # the capture form the program was built with (attn_capture): the launch its captured layers emit, the layout of a call
        self.store_dt = 0    # storage type the conv TOWER keeps its maps in (set by the engine in the 16-bit modes: 1 bf16, 2 f16)
        self.in_fork = False
        self.nbytes = 0
        self._snap = None       # (pending, lane_pool) as of the last records(), until all_waited()
        self._next_slot = -1    # record slot handed out last (records)
        self._c_ops = None      # the launch list as the library reads it (finalize)
        self._flags_op = None   # index of the OP_LANE_FLAGS op, if the program forks
        self.uses_lanes = False
        self.device_sync = False  # the last run() used the device-side fork / join / record / wait
        self._flags = None      # flag buffer of the device-side sync form (_lane_flags)
        self._events = None     # the program's own fork / join / record events (_own_events)
        self._tev = None        # timing events of _run_timed
        self._capture_ws = None  # per-call tensors of bind_capture, held until the next call

    # ---- buffers ----
    def alloc(self, n, h, w, c, dt=0):
        cs = _r16(c)
        numel = (n * h * w * cs + 1) // 2 if dt else n * h * w * cs  # float32 words of storage
        # inside a fork region a lane first re-uses what IT released (same stream: ordered), then buffers freed before the fork
        lst = (self.lane_pool.get((self.lane_ctx, numel)) if self.in_fork else None) or self.pool.get(numel)
        if lst:
            t = lst.pop()
        else:
            t = torch.empty(numel, dtype=torch.float32, device=self.device)
            self.nbytes += numel * 4
            self.keep.append(t)
        return Act(t, n, h, w, c, cs, dt)

    def release(self, *acts):
        for a in acts:
            if a is None:  # (a tower output nobody asked for: HRNetW48.emit(need=...))
                continue
            if self.in_fork:
                self.lane_pool.setdefault((self.lane_ctx, a.t.numel()), []).append(a.t)
            else:
                self.pool.setdefault(a.t.numel(), []).append(a.t)

    def release_deferred(self, *acts):
        """buffers that SEVERAL lanes of the current fork region read (the branch outputs under the fuse layers): reusable only after
        every lane is ordered behind those reads -- behind the next round of records and waits (all_waited) or the join"""
        for a in acts:
            if self.in_fork:
                self.pending.append(a.t)
            else:
                self.pool.setdefault(a.t.numel(), []).append(a.t)

    # ---- ops ----
    def stem(self, st, n, h, w, in_ptr=0, lane=0, n_src=None, out_dt=0):
        """n_src < n: crops n_src.. are computed from the mirrored input (flip test batched into the same forward)."""
        out = self.alloc(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, st["cout"], out_dt)
        self.keep.append(st)
        ns = n if n_src is None else n_src
        a = cabi.StemArgs(in_ptr, st["w"].data_ptr(), st["bias"].data_ptr(), out.ptr, n, st["cin"], h, w, st["cout"], out.cs, ns, ns, out_dt)
        self.ops.append((cabi.OP_STEM, lane, a))
        return out, a

    def pe_res_stem(self, st, n, h, w, lane=0, n_src=None):
        out = self.alloc(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, st["cout"])
        self.keep.append(st)
        ns = n if n_src is None else n_src
        a = cabi.PeResArgs(0, st["w_pre"].data_ptr(), st["w7"].data_ptr(), st["bias"].data_ptr(), out.ptr, n, h, w, st["cout"], out.cs, ns, ns)
        self.ops.append((cabi.OP_PE_RES_STEM, lane, a))
        return out, a

    def conv(self, x, pc, relu=False, res1=None, res2=None, res_post=None, in2=None, up=1, out=None, out_step=1,
             out_off=(0, 0), out_hw=None, lane=0, group=None, act=None, out_dt=None, fuse_in=None):
        """out_dt: storage type of a newly allocated output (default: the input's, so a 16-bit tower stays 16-bit; pass 0 where the
        consumer is an fp32 kernel: encoder, max-pool, head, ...)
        fuse_in = (terms, y): the conv's input is ReLU((x + up(terms[0])) + up(terms[1])) -- fuse_up_add(x, terms, y) folded into the
        staging of an fp32 Winograd conv (fuse_in_ok), which also writes that map to y; y must be a buffer of its own"""
        assert x.cs >= pc.cin_pad and x.c == pc.cin, "conv input channels %d/%d vs weight %d" % (x.c, x.cs, pc.cin)
        assert x.dt in (0, pc.dtype), "16-bit stored input needs the matching 16-bit conv (input %d, conv %d)" % (x.dt, pc.dtype)
        if (LP1X1 and pc.w_lp1 is not None and fuse_in is None and group is None and in2 is None and up == 1 and out_step == 1 and tuple(out_off) == (0, 0)
                and out_hw is None and x.n * x.h * x.w <= LP1X1_MAX_PIX and (out is None or (out.n, out.h, out.w) == (x.n, x.h, x.w))
                # (the kernel's own limits, i2r_conv1x1_lp: whole output rows of cout_pad channels, residual rows laid out like the output)
                and (out is None or out.cs >= pc.cout_pad) and all(r is None or out is None or r.cs == out.cs for r in (res1, res2, res_post))
                and all(r is None or r.cs >= pc.cout_pad for r in (res1, res2, res_post))):
            return self.conv1x1_lp(x, pc, relu=relu, res1=res1, res2=res2, res_post=res_post, out=out, lane=lane, act=act, out_dt=out_dt)
        k = pc.ksize
        if pc.stride == 1:
            conv_h, conv_w = x.h, x.w  # 'same' geometry for 1x1 / 3x3 pad 1 / deconv parity 2x2
        else:
            conv_h, conv_w = (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1
        if up > 1:
            out_step = up
        if out is None:
            oh, ow = out_hw if out_hw else (conv_h * out_step, conv_w * out_step)
            out = self.alloc(x.n, oh, ow, pc.cout, x.dt if out_dt is None else out_dt)
        assert out.cs >= pc.cout_pad or out.cs >= pc.cout
        assert out.dt in (0, pc.dtype) and all(r is None or r.dt == out.dt for r in (res1, res2, res_post)), "residuals share the output's storage type"
        self._check_like(out, res1, res2, res_post)
        if in2 is not None and (in2.n, in2.h, in2.w, in2.cs) != (x.n, x.h, x.w, x.cs):
            raise ValueError("conv second input is [%d, %d, %d, cs %d], the first [%d, %d, %d, cs %d]" % (in2.n, in2.h, in2.w, in2.cs, x.n, x.h, x.w, x.cs))
        self.keep.append(pc)  # the descriptor holds raw pointers: keep the packed weights alive with the program
        d = cabi.ConvDesc()
        d.in_, d.in2, d.w, d.bias = x.ptr, (in2.ptr if in2 is not None else None), pc.w.data_ptr(), pc.bias.data_ptr()
        d.res1 = res1.ptr if res1 is not None else None
        d.res2 = res2.ptr if res2 is not None else None
        d.res_post = res_post.ptr if res_post is not None else None
        d.out = out.ptr
        d.n_img, d.in_h, d.in_w, d.in_cs, d.cin = x.n, x.h, x.w, x.cs, pc.cin_pad
        d.conv_h, d.conv_w, d.out_h, d.out_w, d.out_cs = conv_h, conv_w, out.h, out.w, out.cs
        d.cout, d.cout_pad, d.stride, d.iy0, d.ix0 = pc.cout, pc.cout_pad, pc.stride, pc.iy0, pc.ix0
        d.ntaps = len(pc.taps)
        for i, (dy, dx) in enumerate(pc.taps):
            d.dy[i], d.dx[i] = dy, dx
        d.out_step, d.out_off_y, d.out_off_x, d.rep = out_step, out_off[0], out_off[1], up
        d.relu = int(relu) if act is None else act  # 0 none, 1 ReLU, 2 GELU
        d.dtype = pc.dtype
        d.in_f16, d.out_f16 = int(x.dt != 0), int(out.dt != 0)
        wino = (WINOGRAD and pc.w_wino is not None and pc.dtype == 0 and in2 is None and up == 1 and out_step == 1 and tuple(out_off) == (0, 0)
                and (out.h, out.w) == (conv_h, conv_w) and d.relu in (0, 1))
        if fuse_in is not None:
            terms, y = fuse_in
            if not (wino and self.fuse_in_ok(x, terms, pc)):
                raise ValueError("fuse_in needs an fp32 Winograd conv over every channel of x and 1 or 2 terms at 1/2 or 1/4 of its map")
            assert all(t.cs == x.cs and t.dt == 0 and t.n == x.n for t in terms) and (y.n, y.h, y.w, y.cs, y.dt) == (x.n, x.h, x.w, x.cs, 0)
            sh = [{2: 1, 4: 2}[x.h // t.h] for t in terms]
            assert all((t.h << k, t.w << k) == (x.h, x.w) for t, k in zip(terms, sh))
            d.t1, d.t1_shift, d.y = terms[0].ptr, sh[0], y.ptr
            if len(terms) > 1:
                d.t2, d.t2_shift = terms[1].ptr, sh[1]
        if wino:
            # Winograd F(2x2, 3x3): 2.25x fewer matrix-pipe operations (csrc/i2r_conv_wino.hip); NT 3 or 4, two fragments per workgroup
            nfrag = pc.cout_pad // 16
            nt = 3 if nfrag % 3 == 0 else 4
            fw, fh = wino_fragment(conv_h, conv_w)
            d.algo, d.w = 1, pc.w_wino.data_ptr()
            mt = 1  # one fragment per item: 114 registers = 4 waves per SIMD (measured faster than two fragments at 2 waves per SIMD)
            d.tile_h, d.tile_w, d.mt, d.wn, d.ck = fh, fw, mt, 1, 0
            d.seq = 0 if WINO_SEQ else 1
            push_wino_forms()
            n_frag = x.n * -(-conv_h // fh) * -(-conv_w // fw)
            geo = ("wino", -(-n_frag // mt) * (nfrag // nt))
            key = ("wino", nt, mt)
        else:
            nt, wn = conv_split(pc.cout_pad)
            n_cblk = (pc.cout_pad // 16) // (nt * wn)
            max_d = max(max(t) for t in pc.taps)
            # stride-2 convs stage four input pixels per output pixel: one fragment per wave and three or more workgroups per CU
            # hide that staging (tools/sweep_conv.py at 16 crops: 64->64 s2 82 -> 43 us, 256->96 s2 77 -> 67 us); the cost model's
            # rounds-of-256-workgroups term was fitted on stride-1 shapes
            th, tw, mt = choose_tile(conv_h, conv_w, 4 // wn, pc.stride, max_d, x.n, n_cblk, force_mt=1 if pc.stride == 2 else 0)
            d.tile_h, d.tile_w, d.mt, d.wn, d.ck = th, tw, mt, wn, 0
            geo = (conv_h, conv_w, 4 // wn, pc.stride, max_d, x.n, n_cblk)
            key = nt
        if group is not None:
            group.append((d, geo, key))
        elif wino:  # (a Winograd conv always goes out with its LPT dispatch table: one-member group)
            self.flush_group([(d, geo, key)], lane=lane)
        else:
            self.ops.append((cabi.OP_CONV, lane, d))
        return out

    @staticmethod
    def fuse_in_ok(x, terms, pc):
        """can conv(x, pc, fuse_in=(terms, y)) fold the closing pass?  fp32 Winograd only (csrc/i2r_conv_wino.hip), reading every channel of
        x (so that y comes out complete), one or two terms at half or a quarter of the map"""
        return (WINOGRAD and pc.w_wino is not None and pc.dtype == 0 and x.dt == 0 and x.c == pc.cin and x.cs == pc.cin_pad
                and 1 <= len(terms) <= 2 and all((t.h * 2, t.w * 2) == (x.h, x.w) or (t.h * 4, t.w * 4) == (x.h, x.w) for t in terms))

    @staticmethod
    def _group_tiles(group):
        """common mt + per-member tiles of a grouped launch (cost model: workgroups of all members share the chip)"""
        best = None
        # (all members: with 1x1 members in the group -- the fuse layers' second launch -- forcing it measured -0.7 % on the fp32 tower, +1.5 % on the bf16 one)
        s2 = all(geo[3] == 2 for _, geo, _ in group)
        for mt in ((1,) if s2 else (2, 3, 4, 1)):
            try:
                tiles = [choose_tile(*geo, force_mt=mt, want_cost=True) for _, geo, _ in group]
            except AssertionError:
                continue
            # one launch: workgroups of all members share the chip -> rounds over the SUM of workgroups
            blocks = 0
            work = 0.0
            for (d, geo, _), t in zip(group, tiles):
                conv_h, conv_w, wm, stride, max_d, n_img, n_cblk = geo
                nb = -(-conv_h // t[1]) * -(-conv_w // t[2]) * n_img * n_cblk
                blocks += nb
                work += nb * (wm * mt * 16 / _MT_EFF[mt]) * d.cin * d.ntaps
            cost = work * max(1.0, 256.0 / blocks)
            if best is None or cost < best[0]:
                best = (cost, mt, tiles)
        _, mt, tiles = best
        return mt, tiles

    def flush_group(self, group, lane=0):
        """Emit the convs collected in `group` as ONE grouped launch (same NT required; a common mt is chosen by the
        cost model; heaviest-K members first so the long workgroups start early)."""
        if not group:
            return
        nts = {g[2] for g in group}
        wino = group[0][0].algo == 1  # (the group key keeps the two algorithms apart)
        if (len(group) == 1 and not wino) or len(nts) != 1 or len(group) > cabi.MAX_GROUP:
            # (no common fragment blocking, or more members than a launch holds: sequential launches.  The shipped HRNet towers have
            #  <= 3 branches, whose levels stay within MAX_GROUP; a 4-branch module would land here for its 6-member fuse level)
            for m in list(group):
                if m[0].algo == 1:
                    self.flush_group([m], lane=lane)
                else:
                    self.ops.append((cabi.OP_CONV, lane, m[0]))
            del group[:]
            return
        if not wino:
            mt, tiles = self._group_tiles(group)
        order = sorted(range(len(group)), key=lambda i: -(group[i][0].cin * group[i][0].ntaps))
        a = cabi.ConvGroupArgs()
        counts, works = [], []
        for slot, i in enumerate(order):
            d, geo, _ = group[i]
            a.d[slot] = C.pointer(d)
            self.keep.append(d)
            if wino:
                counts.append(geo[1])
            else:
                d.tile_h, d.tile_w, d.mt = tiles[i][1], tiles[i][2], mt
                conv_h, conv_w, wm, stride, max_d, n_img, n_cblk = geo
                counts.append(-(-conv_h // d.tile_h) * -(-conv_w // d.tile_w) * n_img * n_cblk)
            works.append(d.cin * d.ntaps)
        a.n = len(group)
        if not wino and len(set(works)) > 1:  # dispatch order: heaviest items first, balanced over the CUs
            bm = lpt_block_table(self.device, counts, works)
            self.keep.append(bm)
            a.block_map, a.map_len = bm.data_ptr(), bm.numel()
        self.ops.append((cabi.OP_CONV_GROUP, lane, a))
        del group[:]

    def channel_slice(self, a, c0, c):
        """channels c0 .. c0+c of buffer `a` as an Act of its own (same pixel stride): lets one conv write, and another read, a part
        of a concatenated map.  Never release a slice -- release the parent."""
        assert c0 % 16 == 0 and c0 + c <= a.cs
        words = c0 // 2 if a.dt else c0  # float32 words of storage per channel offset (16-bit maps: two channels per word)
        return Act(a.t[words:], a.n, a.h, a.w, c, a.cs, a.dt)

    def stem_conv2_layer1(self, a, conv2, blocks):
        """Second stem conv + layer1's Bottlenecks (hrnet.py:419-427 / hrformer.py forward).  The first Bottleneck's identity path is a
        1x1 conv + BN of the block input x; its sum with conv3(t2) is ONE 1x1 conv over the concatenation [x ; t2] (Packer.conv_cat):
        conv2 and the block's 3x3 conv write the two halves of one buffer, so the 256-channel downsample map is neither written nor
        read back (one launch and 2 x 3.1 MB per crop less)."""
        first = blocks[0]
        assert "c3ds" in first, "layer1.0 carries the downsample"
        cx, cm = conv2.cout, first["c2"].cout
        cat = self.alloc(a.n, (a.h - 1) // 2 + 1, (a.w - 1) // 2 + 1, cx + cm, a.dt)
        x, t2 = self.channel_slice(cat, 0, cx), self.channel_slice(cat, cx, cm)
        self.conv(a, conv2, relu=True, out=x)
        self.release(a)
        t1 = self.conv(x, first["c1"], relu=True)
        self.conv(t1, first["c2"], relu=True, out=t2)
        def pair_ok(pa, pb):
            """shape limits of i2r_conv1x1_pair (csrc/i2r_conv1x1.hip): K of the first conv 64 | 128, its outputs in whole 32-channel steps,
            the second conv 64 wide; anything else takes the generic conv path below"""
            return (pa.w_frag is not None and pa.cin in (64, 128) and pa.cout % 32 == 0 and pa.cout == pa.cout_pad
                    and (pb is None or (pb.w_frag is not None and pb.cout == 64 and pb.cin == pa.cout)))
        nxt = [b["c1"] for b in blocks[1:]] + [None]
        if PAIR1X1 and a.dt == 0 and pair_ok(first["c3ds"], nxt[0]) and all(pair_ok(b["c3"], nxt[i]) for i, b in enumerate(blocks[1:], 1)):
            # conv3 (+ residual + ReLU) of a block and conv1 (+ ReLU) of the next one in ONE launch: the 256-channel map is written once
            # (it is the next residual) and not read back by conv1
            self.release(t1)
            y, t1 = self.conv1x1_pair(cat, first["c3ds"], None, blocks[1]["c1"] if len(blocks) > 1 else None)
            self.release(cat)
            for i, blk in enumerate(blocks[1:], 1):
                t2 = self.conv(t1, blk["c2"], relu=True)
                self.release(t1)
                yn, t1 = self.conv1x1_pair(t2, blk["c3"], y, blocks[i + 1]["c1"] if i + 1 < len(blocks) else None)
                self.release(t2, y)
                y = yn
            return y
        y = self.conv(cat, first["c3ds"], relu=True)
        self.release(t1, cat)
        x = y
        for blk in blocks[1:]:
            t1 = self.conv(x, blk["c1"], relu=True)
            t2 = self.conv(t1, blk["c2"], relu=True)
            y = self.conv(t2, blk["c3"], relu=True, res1=x)
            self.release(t1, t2, x)
            x = y
        return x

    def deconv(self, x, pcs, relu=True, res_post=None, lane=0):
        """ConvTranspose(k4,s2,p1)+BN(+ReLU)(+post-ReLU residual) as four parity convs writing the interleaved 2x output."""
        out = self.alloc(x.n, 2 * x.h, 2 * x.w, pcs[(0, 0)].cout, x.dt)
        # the four parities are independent convs of one shape over the same input: ONE grouped launch (each alone is a
        # few hundred small workgroups -- 16 us at 27 TFLOP/s on the 16x12 map at 32 crops)
        grp = []
        for (py, px), pc in pcs.items():
            self.conv(x, pc, relu=relu, res_post=res_post, out=out, out_step=2, out_off=(py, px), lane=lane, group=grp)
        self.flush_group(grp, lane=lane)
        return out

    def rows_gather(self, src, crop_map, lane=0):
        """[len(crop_map), h, w, c] whose crop i is crop crop_map[i] of src, zeros for -1 (padding_tensor: the padded persons as rows)"""
        out = self.alloc(len(crop_map), src.h, src.w, src.c)
        assert out.cs == src.cs, "rows_gather copies whole rows: source and output need the same row stride (%d vs %d)" % (src.cs, out.cs)
        m = torch.tensor(list(crop_map), dtype=torch.int32).to(self.device)
        self.keep.append(m)
        a = cabi.GatherArgs(src.ptr, out.ptr, m.data_ptr(), len(crop_map), src.h * src.w * src.cs)
        self.ops.append((cabi.OP_ROWS_GATHER, lane, a))
        return out

    def rows_gather_multi(self, segments, lane=0):
        """ONE launch for up to cabi.MAX_GATHER_SEGS gathers (i2r_rows_gather_multi).  segments: (src, out, table, n_out, n_src, src_crop,
        out_crop) -- crop out_crop + i of `out` = crop src_crop + table[i] of `src` for i < n_out, zeros where table[i] is outside
        [0, n_src).  src, out: Acts, or anything else with ptr, n, h, w, cs, dt (_RawAct: a buffer the program does not own).  Rows of any
        storage type; the device int32 tables belong to the CALLER, who refills them per call and may patch src and n_src of the returned
        args (the launch is fixed, the contents are not).  The output windows must not overlap."""
        assert 1 <= len(segments) <= cabi.MAX_GATHER_SEGS, "rows_gather_multi: %d segments (1..%d)" % (len(segments), cabi.MAX_GATHER_SEGS)
        a = cabi.GatherMultiArgs()
        a.n_seg = len(segments)
        for g, (src, out, table, n_out, n_src, src_crop, out_crop) in zip(a.seg, segments):
            row = src.h * src.w * src.cs * (2 if src.dt else 4)
            assert (out.h, out.w, out.cs, out.dt) == (src.h, src.w, src.cs, src.dt), "rows_gather_multi copies whole rows of one stride and type"
            assert row % 16 == 0 and table.dtype == torch.int32 and table.numel() >= n_out
            assert 0 <= out_crop and out_crop + n_out <= out.n and 0 <= src_crop and src_crop + n_src <= src.n
            self.keep.append(table)
            g.src, g.out, g.map = src.ptr + row * src_crop, out.ptr + row * out_crop, table.data_ptr()
            g.n_out, g.n_src, g.row_bytes = n_out, n_src, row
        self.ops.append((cabi.GROUPS_OP_ROWS_GATHER_MULTI, lane, a))
        return a

    def view_scramble(self, o, person_map, n_images, max_persons, c, lane=0):
        """GeneralTransformerBlock's re-viewing of the attention output (attention.py:1025-1029, i2r_view_scramble) + get_valid_output"""
        out = self.alloc(len(person_map), o.h, o.w, c)
        m = torch.tensor(list(person_map), dtype=torch.int32).to(self.device)
        self.keep.append(m)
        a = cabi.ScrambleArgs(o.ptr, out.ptr, m.data_ptr(), len(person_map), n_images, max_persons, c, out.cs, o.h * o.w)
        assert o.cs == out.cs and o.n == n_images * max_persons
        self.ops.append((cabi.OP_VIEW_SCRAMBLE, lane, a))
        return out

    def pe_cat_vec(self, fc, n, h, w, th, tw, out, c0, lane=0, n_src=None):
        """PositionEmbeddingImage 'cat_vec': one vector per person from the boundary mask [n_src, 1, h, w], written into channels [c0, c0 + vec)
        of every token row of `out` (zeros behind, up to the row stride)"""
        rate = int(math.log(w // tw, 2))
        assert (out.n, out.h, out.w) == (n, th, tw) and out.dt == 0 and c0 + fc["vec"] <= out.cs
        self.keep.append(fc)
        ns = n if n_src is None else n_src
        a = cabi.PeCatVecArgs(0, fc["w"].data_ptr(), fc["b"].data_ptr(), out.ptr, n, h, w, th, tw, rate, fc["vec"], out.cs, c0, out.cs, ns, ns)
        self.ops.append((cabi.OP_PE_CAT_VEC, lane, a))
        return a

    def maxpool(self, x, lane=0, out=None):
        """out: a (wider) destination whose first x.cs channels receive the pooled map (the x half of a channel concatenation)"""
        assert x.dt == 0, "fp32 kernel: the producer must store fp32 (conv(..., out_dt=0))"
        if out is None:
            out = self.alloc(x.n, (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1, x.c)
        assert (out.n, out.h, out.w) == (x.n, (x.h - 1) // 2 + 1, (x.w - 1) // 2 + 1) and out.cs >= x.cs and out.dt == 0
        a = cabi.PoolArgs(x.ptr, out.ptr, x.n, x.h, x.w, x.cs, x.cs, out.cs)  # pool all cs channels (pads stay 0)
        self.ops.append((cabi.OP_MAXPOOL, lane, a))
        return out

    def layernorm(self, x, ln, eps=1e-6, lane=0, out_dt=0):
        """out_dt: storage type of the normalised map (16-bit modes: it only feeds a 16-bit conv)"""
        assert x.dt == 0, "fp32 kernel: the producer must store fp32 (conv(..., out_dt=0))"
        out = self.alloc(x.n, x.h, x.w, x.c, out_dt)
        self.keep.append(ln)
        a = cabi.LnArgs(x.ptr, ln["w"].data_ptr(), ln["b"].data_ptr(), out.ptr, x.n * x.h * x.w, x.c, x.cs, eps, out_dt)
        self.ops.append((cabi.OP_LAYERNORM, lane, a))
        return out

    def winattn(self, qkv, bias, c, heads, lane=0):
        hs = heads * Packer.HEAD_PAD
        assert qkv.cs == 3 * hs, (qkv.cs, hs)
        out = self.alloc(qkv.n, qkv.h, qkv.w, hs)  # head-padded channels (consumed by Packer.attn_out)
        self.keep.append(bias)
        a = cabi.WinAttnArgs(qkv.ptr, bias.data_ptr(), out.ptr, qkv.n, qkv.h, qkv.w, c, hs, heads)
        self.ops.append((cabi.OP_WINATTN, lane, a))
        return out

    def hrt_attn(self, x, ab, eps=1e-6, lane=0, variant=None):
        """fused x + out_proj(window_attn(qkv(LN1 x))) (16-bit modes, i2r_hrt_attn_block); variant: None / 0 = the library's choice,
        1 wave per token tile, 2 wave per head"""
        assert x.dt == 0 and x.c == ab["c"] and x.cs == ab["cs"]
        if not variant or (variant == 1 and ab["c"] not in (78, 156)):
            variant = 2  # measured (tools/time_hrt_attn.py, 16 crops bf16): wave per head 20.4 / 19.3 us against 25.6 / 30.2 us (C = 78 / 156)
        out = self.alloc(x.n, x.h, x.w, x.c)
        self.keep.append(ab)
        a = cabi.HrtAttnArgs(x.ptr, out.ptr, ab["ln"]["w"].data_ptr(), ab["ln"]["b"].data_ptr(), ab["wqkv"].data_ptr(), ab["bqkv"].data_ptr(),
                             ab["wo"].data_ptr(), ab["bo"].data_ptr(), x.n, x.h, x.w, x.c, x.cs, ab["heads"], eps, ab["dtype"], variant)
        self.ops.append((cabi.OP_HRT_ATTN, lane, a))
        return out

    def hrt_mlp(self, x, mb, eps=1e-6, lane=0, variant=None):
        """fused x + mlp(LN2 x) (16-bit modes, i2r_hrt_mlp_block); variant: None / 0 = the measured choice per width (_MLP_VARIANT),
        1 fc2 accumulated per wave, 2 fc2 by output-block ownership"""
        assert x.dt == 0 and x.c == mb["c"] and x.cs == mb["cs"]
        if not variant or (variant == 1 and mb["c"] > 156):
            variant = _MLP_VARIANT[mb["c"]]
        out = self.alloc(x.n, x.h, x.w, x.c)
        self.keep.append(mb)
        a = cabi.HrtMlpArgs(x.ptr, out.ptr, mb["ln"]["w"].data_ptr(), mb["ln"]["b"].data_ptr(), mb["w1"].data_ptr(), mb["b1"].data_ptr(),
                            mb["wdw"].data_ptr(), mb["bdw"].data_ptr(), mb["w2"].data_ptr(), mb["b2"].data_ptr(), x.n, x.h, x.w, x.c, x.cs,
                            mb["hidden_pad"], eps, mb["dtype"], variant)
        self.ops.append((cabi.OP_HRT_MLP, lane, a))
        return out

    def dwconv(self, x, dw, stride=1, act=0, lane=0):
        """the output keeps the input's storage type (stride 1: fp32 or 16 bit; stride 2: fp32 only)"""
        assert x.dt == 0 or stride == 1
        assert x.c == dw["c"] and x.cs == dw["cs"]
        out = self.alloc(x.n, (x.h - 1) // stride + 1, (x.w - 1) // stride + 1, x.c, x.dt)
        self.keep.append(dw)
        a = cabi.DwArgs(x.ptr, dw["w"].data_ptr(), dw["bias"].data_ptr(), out.ptr, x.n, x.h, x.w, x.c, x.cs, stride, act, x.dt)
        self.ops.append((cabi.OP_DWCONV, lane, a))
        return out

    def upsample_add(self, low, res, out, act=0, lane=0):
        """out = act(((res + up(low_0)) + up(low_1)) + up(low_2)): bilinear up-sampling of 1..3 lower-resolution maps (an Act or a list
        of Acts, added in that order) in one pass (i2r_upsample_bilinear_add_multi)"""
        lows = list(low) if isinstance(low, (list, tuple)) else [low]
        assert 1 <= len(lows) <= 3
        sc = [out.h // t.h for t in lows]
        assert all(t.h * s == out.h and t.w * s == out.w and t.cs == out.cs == res.cs and t.n == out.n for t, s in zip(lows, sc))
        a = cabi.UpArgs(lows[0].ptr, res.ptr, out.ptr, lows[0].n, lows[0].h, lows[0].w, sc[0], lows[0].c, lows[0].cs, act,
                        lows[1].ptr if len(lows) > 1 else None, lows[2].ptr if len(lows) > 2 else None,
                        sc[1] if len(lows) > 1 else 1, sc[2] if len(lows) > 2 else 1)
        self.ops.append((cabi.OP_UPSAMPLE, lane, a))
        return out

    @staticmethod
    def _check_like(out, *residuals):
        """the kernels index a residual like the output: a smaller map would be read out of bounds (e.g. a 2-stage config whose up-sampled
        map is not the first stage's size -- the reference fails on that sum too)"""
        for r in residuals:
            if r is not None and (r.n, r.h, r.w, r.cs) != (out.n, out.h, out.w, out.cs):
                raise ValueError("conv residual is [%d, %d, %d, row %d], the output [%d, %d, %d, row %d]" % (r.n, r.h, r.w, r.cs, out.n, out.h, out.w, out.cs))

    def conv1x1_lp(self, x, pc, relu=False, res1=None, res_post=None, out=None, lane=0, act=None, out_dt=None, res2=None):
        """single 1x1 conv over few pixels in the 16-bit modes (i2r_conv1x1_lp: operands straight from global memory, K split over the
        workgroup's waves); same semantics as conv(): out = act(W x + b + res1) + res_post"""
        if out is None:
            out = self.alloc(x.n, x.h, x.w, pc.cout, x.dt if out_dt is None else out_dt)
        assert out.cs >= pc.cout_pad and out.dt in (0, pc.dtype) and all(r is None or (r.dt == out.dt and r.cs == out.cs) for r in (res1, res2, res_post))
        self._check_like(out, res1, res2, res_post)
        self.keep.append(pc)
        a = cabi.Conv1x1LpArgs(x.ptr, pc.w_lp1.data_ptr(), pc.bias.data_ptr(), res1.ptr if res1 is not None else None,
                               res_post.ptr if res_post is not None else None, out.ptr, x.n * x.h * x.w, pc.cin_pad, pc.cout_pad, x.cs, out.cs,
                               (int(relu) if act is None else act), pc.dtype, int(x.dt != 0), int(out.dt != 0), 0,
                               res2.ptr if res2 is not None else None)
        self.ops.append((cabi.OP_CONV1X1_LP, lane, a))
        return out

    def conv1x1_pair(self, x, pa, res, pb, lane=0):
        """y = ReLU(conv1x1_a(x) [+ res]) and, with pb, z = ReLU(conv1x1_b(y)) in one launch (i2r_conv1x1_pair) -> (y, z | None)"""
        assert x.dt == 0 and pa.w_frag is not None and pa.ksize == 1 and pa.cin == x.cs and (pb is None or (pb.w_frag is not None and pb.cin == pa.cout))
        y = self.alloc(x.n, x.h, x.w, pa.cout)
        z = self.alloc(x.n, x.h, x.w, pb.cout) if pb is not None else None
        assert res is None or (res.cs == y.cs and res.dt == 0 and res.n * res.h * res.w == y.n * y.h * y.w)
        self.keep.extend([pa, pb])
        a = cabi.Conv1x1PairArgs(x.ptr, pa.w_frag.data_ptr(), pa.bias.data_ptr(), res.ptr if res is not None else None, y.ptr,
                                 pb.w_frag.data_ptr() if pb is not None else None, pb.bias.data_ptr() if pb is not None else None,
                                 z.ptr if z is not None else None, x.n * x.h * x.w, pa.cin, pa.cout, pb.cout if pb is not None else 0,
                                 x.cs, y.cs, z.cs if z is not None else 0, 1, 1, 0)
        self.ops.append((cabi.OP_CONV1X1_PAIR, lane, a))
        return y, z

    def fuse_up_add(self, base, terms, out, relu=True, lane=0):
        """out = act((base + up(t1)) + up(t2)): nearest-neighbour up-sampled low-resolution terms added in one HBM-bound pass
        (i2r_fuse_up_add); terms: 1 or 2 Acts whose maps are base's divided by a power of two"""
        assert 1 <= len(terms) <= 2 and all(t.cs == base.cs == out.cs and t.dt == base.dt == out.dt and t.n == base.n for t in terms)
        sc = [base.h // t.h for t in terms]
        assert all(t.h * s == base.h and t.w * s == base.w for t, s in zip(terms, sc))
        a = cabi.FuseUpArgs(base.ptr, terms[0].ptr, terms[1].ptr if len(terms) > 1 else None, out.ptr, base.n, base.h, base.w, base.cs,
                            sc[0], sc[1] if len(terms) > 1 else 1, int(relu), base.dt)
        self.ops.append((cabi.OP_FUSE_UP, lane, a))
        return out

    def head(self, x, hd, out_ptr=0, lane=0):
        assert x.dt == 0, "fp32 kernel: the producer must store fp32 (conv(..., out_dt=0))"
        self.keep.append(hd)
        tmp = None
        if hd.get("conv3") is not None:  # FINAL_CONV_KERNEL 3: the conv kernel does the 3x3 (+ bias), i2r_head only transposes to NCHW
            x = tmp = self.conv(x, hd["conv3"], out_dt=0, lane=lane)
        a = cabi.HeadArgs(x.ptr, hd["w"].data_ptr(), hd["bias"].data_ptr(), out_ptr, x.n, x.h, x.w, hd["cin"], x.cs, hd["cout"])
        self.ops.append((cabi.OP_HEAD, lane, a))
        if tmp is not None:
            self.release(tmp)
        return a

    def encoder(self, x, layers, grp_off_host, pos=None, pos_period=0, lane=0, regroupable=False, pre_norm=False, pos_table=None, capture=None):
        """x: Act viewed as tokens [n*h*w, cs]; grp_off_host: python list of token offsets per group.
        regroupable: the grouping (persons per image) may be changed later with set_groups() without rebuilding the program:
        the offset table gets capacity for one group per crop.
        capture: dict(stack=state-dict prefix, layers={i: fp32 Packer.encoder_layer_mh pack of layer i}) -- the attention maps of those
        layers are computed too (the launch of the program's capture form, emitted before the layer's input is released); see bind_capture."""
        assert x.dt == 0, "the encoder kernels read fp32 token rows"
        if layers and layers[0].get("mh"):
            return self.encoder_mh(x, layers, grp_off_host, pos=pos, pos_period=pos_period, lane=lane, regroupable=regroupable, pre_norm=pre_norm,
                                   pos_table=pos_table, capture=capture)
        assert not pre_norm, "the fused layer kernels are post-norm"
        cap = self._capture_begin(capture, x)
        pos_act = self._pos_rows(x, pos, pos_period, pos_table) if cap is not None else None
        n_tok = x.n * x.h * x.w
        cs = x.cs
        n_pad = (n_tok + 63) // 64 * 64 + 64
        # fp32 mode: the K/V projection of layer i+1 is fused into the tail of layer i (ping-pong K/V buffers); the 16-bit
        # capable stacks keep one enc_kv launch per layer (they may fall back to fp32 kernels per call, see set_groups)
        fuse_kv = all(not L.get("dtype", 0) for L in layers) and len(layers) > 1
        nbuf = 2 if fuse_kv else 1
        # K / V^T workspaces: fragment-packed per 16-token tile of a group (fp32 kernels; <= n_tok/16 + groups tiles) or the
        # 16-bit kernels' [n_tok, cs] / [cs, n_pad] images -- sized for either
        kv_floats = max((n_tok // 16 + x.n + 1) * 16 * cs, (n_tok // 32 + x.n + 1) * 32 * 96 // 2)
        kbufs = [torch.zeros(kv_floats, dtype=torch.float32, device=self.device) for _ in range(nbuf)]
        vbufs = [torch.zeros(kv_floats, dtype=torch.float32, device=self.device) for _ in range(nbuf)]
        goff = torch.zeros(x.n + 1, dtype=torch.int32, device=self.device)
        # hand-off scratch of the partial key split (launches with 256 < tiles < 512; include/i2r_hip.h): <= 256 split tiles
        split_ws = torch.empty(256 * 2 * 1792, dtype=torch.float32, device=self.device)
        split_cnt = torch.zeros(256, dtype=torch.int32, device=self.device)
        self.keep += kbufs + vbufs + [goff, split_ws, split_cnt]
        self.nbytes += sum(t.numel() * t.element_size() for t in kbufs + vbufs + [goff, split_ws, split_cnt])
        self.split_counters.append(split_cnt)
        cur = x
        self.keep.append(layers)
        descs = []
        for i, L in enumerate(layers):
            assert L["cs"] == cs
            if cap is not None and i in capture["layers"]:  # q|k of the fused layer's input, projected again in fp32 (the fused kernels keep it on chip)
                mh = capture["layers"][i]
                qk = self.conv(cur, mh["qk"], in2=pos_act, lane=lane)
                if not self._capture_layer(cap, i, qk, mh, goff, lane):
                    self.release(qk)
            out = self.alloc(x.n, x.h, x.w, x.c)
            d = cabi.EncoderDesc()
            d.src, d.pos = cur.ptr, (pos if pos else None)
            d.kbuf, d.vbuf, d.out, d.grp_off = kbufs[i % nbuf].data_ptr(), vbufs[i % nbuf].data_ptr(), out.ptr, goff.data_ptr()
            for name in ("w_in", "b_in", "w_out", "b_out", "ln1_w", "ln1_b", "w1", "b1", "w2", "b2", "ln2_w", "ln2_b"):
                setattr(d, name, L[name].data_ptr())
            d.n_tok, d.d, d.cs, d.dff_pad = n_tok, L["d"], cs, L["dff_pad"]
            d.pos_period, d.ln_eps = pos_period, 1e-5
            d.split_ws, d.split_cnt = split_ws.data_ptr(), split_cnt.data_ptr()
            if L.get("dtype", 0):
                d.w_in_lp, d.w_out_lp, d.w1_lp, d.w2_lp, d.vec_lp = (L[k].data_ptr() for k in ("w_in_lp", "w_out_lp", "w1_lp", "w2_lp", "vec_lp"))
            if fuse_kv and i + 1 < len(layers):
                nxt = layers[i + 1]
                d.next_w_in, d.next_b_in = nxt["w_in"].data_ptr(), nxt["b_in"].data_ptr()
                d.next_kbuf, d.next_vbuf = kbufs[(i + 1) % nbuf].data_ptr(), vbufs[(i + 1) % nbuf].data_ptr()
            descs.append((d, L.get("dtype", 0)))
            if i == 0 or not fuse_kv:
                self.ops.append((cabi.OP_ENC_KV, lane, d))
            self.ops.append((cabi.OP_ENC_LAYER, lane, d))
            if cur is not x:
                self.release(cur)
            cur = out
        self._register_stack(dict(descs=descs, goff=goff, current=None), grp_off_host, cap, x.h * x.w if regroupable else None)
        return cur

    def encoder_mh(self, x, layers, grp_off_host, pos=None, pos_period=0, lane=0, regroupable=False, pre_norm=False, pos_table=None, capture=None):
        """The general encoder stack (Packer.encoder_layer_mh): per layer, post-norm (forward_post, attention.py:61-82)
            q|k = (src + pos) Wqk ; v = src Wv ; a = mh_attention ; x = LN1(src + a Wo) ; out = LN2(x + W2 relu(W1 x))
        or pre-norm (forward_pre, attention.py:84-103: q and k from LN1(src) + pos, the VALUE from src itself)
            q|k = (LN1(src) + pos) Wqk ; v = src Wv ; x = src + a Wo ; out = x + W2 relu(W1 LN2(x)).
        pos: device address of per-token rows laid out like x, or of a [pos_period, cs] table (TransPose-H), or 0.
        capture: as for encoder(); the maps are read from each captured layer's own q|k activation."""
        pos_act = self._pos_rows(x, pos, pos_period, pos_table)
        goff = torch.zeros(x.n + 1, dtype=torch.int32, device=self.device)
        self.keep += [goff, layers]
        self.nbytes += goff.numel() * 4
        cap = self._capture_begin(capture, x)
        cur, mh_args = x, []
        for i, L in enumerate(layers):
            assert L["cs"] == x.cs
            qk_in = self.layernorm(cur, L["ln1"], eps=1e-5, lane=lane) if pre_norm else cur
            qk = self.conv(qk_in, L["qk"], in2=pos_act, lane=lane)
            held = cap is not None and i in capture["layers"] and self._capture_layer(cap, i, qk, L, goff, lane)
            v = self.conv(cur, L["v"], lane=lane)
            if pre_norm:
                self.release(qk_in)
            att = self.alloc(x.n, x.h, x.w, L["hs"])
            a = cabi.MhAttnArgs(qk.ptr, v.ptr, att.ptr, goff.data_ptr(), 0, L["heads"], L["hp"], L["hs"], qk.cs, v.cs, att.cs, 0, 0, 0)
            self.ops.append((cabi.OP_MH_ATTN, lane, a))
            mh_args.append(a)
            self.release(*((v,) if held else (qk, v)))
            x1 = self.conv(att, L["o"], res1=cur, lane=lane)  # src + attention
            self.release(att)
            if cur is not x:
                self.release(cur)
            if pre_norm:
                n2 = self.layernorm(x1, L["ln2"], eps=1e-5, lane=lane)
                hdn = self.conv(n2, L["w1"], relu=True, lane=lane)
                self.release(n2)
                cur = self.conv(hdn, L["w2"], res1=x1, lane=lane)
                self.release(hdn, x1)
            else:
                n1 = self.layernorm(x1, L["ln1"], eps=1e-5, lane=lane)
                self.release(x1)
                hdn = self.conv(n1, L["w1"], relu=True, lane=lane)
                y = self.conv(hdn, L["w2"], res1=n1, lane=lane)
                self.release(hdn, n1)
                cur = self.layernorm(y, L["ln2"], eps=1e-5, lane=lane)
                self.release(y)
        self._register_stack(dict(descs=[], mh=mh_args, goff=goff, current=None), grp_off_host, cap, x.h * x.w if regroupable else None)
        return cur

    def _register_stack(self, grouping, grp_off_host, cap=None, regroup_tok=None):
        """an emitted encoder stack joins the program: its groups are set, a capture learns its grouping, and with regroup_tok (tokens
        per crop) the engine may regroup it per call (groupings)"""
        self.set_groups(grouping, grp_off_host)
        if cap is not None:
            cap.grouping = grouping
        self.enc_stacks.append(grouping)  # every encoder stack of the program (bench.py: algorithmic FLOPs of the attention blocks)
        if regroup_tok is not None:
            self.groupings.append((grouping, regroup_tok))

    def _pos_rows(self, x, pos, pos_period, pos_table):
        """the position embedding as a second conv input laid out like x (None without one): per-token rows as they are, a [pos_period, cs]
        table (TransPose-H) repeated per crop once at build time"""
        if not pos:
            return None
        if pos_period:
            assert x.h * x.w == pos_period and pos_table is not None and pos_table.data_ptr() == pos and tuple(pos_table.shape) == (pos_period, x.cs)
            rep = pos_table.unsqueeze(0).expand(x.n, pos_period, x.cs).contiguous()
            self.keep.append(rep)
            self.nbytes += rep.numel() * 4
            pos = rep.data_ptr()
        return _RawAct(pos, x)

    # ---- attention maps (capture programs) ----
    # A capture program computes, next to its usual outputs, the attention maps of the requested encoder layers in the form it was built
    # with (attn_capture: full [L, L] maps, rows / columns at query points, reductions per person) into ONE per-call buffer.  The launch list
    # is fixed at build time; bind_capture() patches the per-call part and uploads the offsets of the groups' blocks, like set_groups() does.
    # A deferred form keeps its launches out of the list: the joint form needs the heat maps of the same call, a merged form (the flip
    # test's maps) the q|k of both halves, so the engine issues them behind the run (the form's pair in attn_bind.py) on the q|k the captured layers kept.
    def _capture_begin(self, capture, x):
        if not capture:
            return None
        self.captures.append(self.form.begin(capture["stack"], x, lambda: torch.zeros(x.n, dtype=torch.int64, device=self.device)))
        self.keep += self.captures[-1].off
        return self.captures[-1]

    def _capture_layer(self, cap, i, qk, L, goff, lane):
        """the launch of captured layer i on its q|k activation -> True when q|k must be held (a deferred form), else the caller releases it"""
        assert qk.dt == 0 and qk.cs >= 2 * L["hs"]
        self.keep.append(L)
        kind, a = self.form.launch(cap, qk, L, goff)
        cap.ops.append((i, a))
        if not self.form.behind:  # (else the form's pair runs the launch behind the program: q|k stays out of the pool until the program ends)
            self.ops.append((kind, lane, a))
        return bool(self.form.behind)

    def bind_capture(self, glens, call=None):
        """glens: per capture (program order) the token count of every group to compute (the real images / crops of this call, a prefix of
        the stack's groups); call: the per-call data of the form (AttnQueries: token tables and counts).  -> per block set of the form
        {(stack, layer): per group a view}, all views of one buffer: capture after capture, layer after layer, each as the form's plan
        lays it out."""
        form, plans = self.form, []
        for cap, lens in zip(self.captures, glens):  # the groups asked for are the first groups of the stack as it is grouped now
            cur = cap.grouping["current"]
            assert len(lens) >= 1 and list(lens) == [cur[g + 1] - cur[g] for g in range(len(lens))]
            plans.append(form.plan(cap.stack, (cap.x.h, cap.x.w), lens, max(a.heads for _, a in cap.ops), call))
        form.share(plans)
        buf = (torch.zeros if form.zero_fill else torch.empty)(sum(p.layer_floats * form.sets(cap) + p.extra_floats for p, cap in zip(plans, self.captures)),
                                                               dtype=torch.float32, device=self.device)
        ws = torch.empty(max(p.ws_floats for p in plans), dtype=torch.float32, device=self.device)
        rows = torch.empty(max(p.rows_floats for p in plans), dtype=torch.float32, device=self.device)
        held = [ws, rows]  # (kept until the next call: the launches read them asynchronously; torch's allocator orders reuse by stream)
        views, base = [{} for _ in plans[0].blocks], 0
        for cap, lens, p in zip(self.captures, glens, plans):
            for off, blk in zip(cap.off, p.blocks):
                off[:len(lens)].copy_(torch.tensor(blk.offs[:-1], dtype=torch.int64).pin_memory(), non_blocking=True)
            tables = cap.tables = [t.pin_memory().to(self.device, non_blocking=True) if torch.is_tensor(t) else
                                   torch.empty(t, dtype=torch.int32, device=self.device) for t in p.tables]
            host_off = (C.c_int32 * (len(lens) + 1))(*cap.grouping["current"][:len(lens) + 1])  # (the query and person launches read it)
            held += tables + [host_off]
            ptrs = (ws.data_ptr(), rows.data_ptr(), [t.data_ptr() for t in tables], C.cast(host_off, C.c_void_p))
            cap.base = base
            for n, (i, a) in enumerate(cap.ops):
                form.patch(a, p, buf.data_ptr() + 4 * base, *ptrs)
                if n < form.sets(cap):  # (a roll-out: one set of blocks per stack)
                    for out, blk in zip(views, p.blocks):
                        if blk.shapes:
                            b = base + blk.base
                            out[(cap.stack, i)] = [buf[b + o:b + o + math.prod(s)].view(s) for o, s in zip(blk.offs, blk.shapes)]
                    base += p.layer_floats
            base += p.extra_floats
        if form.behind:  # (the call's part of the work behind the head)
            attn_bind.PAIRS[form.behind][0](self, plans, glens, buf, rows, held, call)
        self._capture_ws = held
        return views

    def set_groups(self, grouping, grp_off_host):
        """(Re)define the token groups of an encoder stack: uploads the offset table and patches the per-layer descriptors."""
        offs = tuple(int(o) for o in grp_off_host)
        if grouping["current"] == offs:
            return
        assert len(offs) <= grouping["goff"].numel()
        lens = [offs[i + 1] - offs[i] for i in range(len(offs) - 1)]
        assert all(l > 0 for l in lens)
        nq, nq16, nq64, nq192 = (sum(-(-l // t) for l in lens) for t in (32, 16, 64, 192))
        # (pinned staging + stream-ordered copy: a pageable source would make every regroup of the validate() loop a blocking copy; torch's
        #  caching host allocator keeps the pinned block alive until the copy has run)
        grouping["goff"][:len(offs)].copy_(torch.tensor(offs, dtype=torch.int32).pin_memory(), non_blocking=True)
        for d, dt in grouping["descs"]:
            d.n_grp, d.n_qtiles32, d.n_qtiles16, d.n_qtiles64 = len(offs) - 1, nq, nq16, nq64
            d.n_qtiles192 = nq192  # (16-bit encoder, long groups: four waves per workgroup share the K / V stream through LDS)
            d.dtype = dt  # (both kernel families take any group offsets: K / V blocks are numbered group by group)
        for a in grouping.get("mh", ()):
            a.n_grp, a.n_qtiles16, a.n_qtiles32, a.n_qtiles64 = len(offs) - 1, nq16, nq, nq64
        grouping["current"] = offs

    def fork(self, mask):
        """lanes in `mask` (bits 1..3) start after everything issued so far on lane 0"""
        if not any(k == cabi.OP_LANE_FLAGS for k, _, _ in self.ops):
            self.ops.append((cabi.OP_LANE_FLAGS, 0, None))  # (run() points it at the flag buffer when the device-side sync form may be used)
        self.ops.append((cabi.OP_FORK, mask, None))
        self.in_fork = True

    def _flush_lane_pools(self):
        for t in self.pending:
            self.pool.setdefault(t.numel(), []).append(t)
        self.pending = []
        for (_, numel), lst in self.lane_pool.items():
            self.pool.setdefault(numel, []).extend(lst)
        self.lane_pool = {}

    # Point-to-point synchronisation inside a fork region (round 6).  `records(lanes)`: every lane puts an event behind what it has issued so
    # far; `wait(lane, slot)`: that lane's stream waits for one of them -- emitted right before the first launch that reads the other
    # lane's data, so a lane starts the terms of the lanes that are done while the last one is still busy (an all-to-all barrier costs
    # every lane ~20 us after the LAST lane ends, tools/probe/xstream_latency2.hip).  Buffers: what the lanes had released when they
    # recorded becomes reusable by every lane at `all_waited()` -- the point of the launch list behind which every lane has waited for
    # every record; what is released after the records waits for the next round.  tests/test_lanes.py replays the happens-before relation.
    def records(self, lanes):
        assert self.in_fork and self._snap is None
        slots, region = {}, 0
        for l in lanes:
            region |= 1 << l
        for l in lanes:  # (every lane of the region waits for every record of the round -- _emit_module makes sure -- so every flag is consumed)
            slot = self._next_slot = (self._next_slot + 1) % 8
            self.ops.append((cabi.OP_RECORD, l | slot << 8 | region << 16, None))
            slots[l] = slot
        self._snap = (self.pending, self.lane_pool)
        self.pending, self.lane_pool = [], {}
        return slots

    def wait(self, lane, slot):
        self.ops.append((cabi.OP_WAIT, lane | slot << 8, None))

    def all_waited(self):
        pend, lp = self._snap
        self._snap = None
        for t in pend:
            self.pool.setdefault(t.numel(), []).append(t)
        for (_, numel), lst in lp.items():
            self.pool.setdefault(numel, []).extend(lst)

    def join(self, mask):
        """lane 0 continues after the lanes in `mask`; buffers freed inside the region become reusable"""
        assert self._snap is None
        self.ops.append((cabi.OP_JOIN, mask, None))
        self.in_fork = False
        self._flush_lane_pools()
        self.lane_ctx = 0

    # ---- run ----
    def finalize(self):
        arr = (cabi.Op * len(self.ops))()
        for i, (kind, lane, st) in enumerate(self.ops):
            arr[i].kind, arr[i].lane = kind, lane
            arr[i].args = C.cast(C.pointer(st), C.c_void_p) if st is not None else None
        self._c_ops = arr
        self._flags_op = next((i for i, (kind, _, _) in enumerate(self.ops) if kind == cabi.OP_LANE_FLAGS), None)
        self.uses_lanes = any(lane != 0 or kind in cabi.SYNC_OPS for kind, lane, _ in self.ops)

    def run(self, side_streams=None, events=None):
        """side_streams: 3 torch.cuda.Stream for lanes 1..3 (None -> everything on the current stream).  A Program owns its
        activation arena and hand-off counters: never replay one Program concurrently on two streams."""
        L = cabi.lib()
        push_wino_forms()
        push_conv_forms()
        cur = torch.cuda.current_stream(self.device).cuda_stream
        if side_streams is None:
            streams = (C.c_void_p * 4)(cur, cur, cur, cur)
        else:
            streams = (C.c_void_p * 4)(cur, *[s.cuda_stream for s in side_streams])
        evs = None
        if self._flags_op is not None:
            # device-side fork / join / record / wait only when every lane stream was PROBED to run beside the caller's stream and beside
            # every other lane (its own hardware queue): a spinning wait kernel must never sit in front of the kernel that signals it
            spin = side_streams is not None and DEVICE_SYNC and lanes_independent(self.device, side_streams, cur)
            self._c_ops[self._flags_op].args = self._lane_flags().data_ptr() if spin else None
            self.device_sync = spin
        if self.uses_lanes:
            if events is None:
                events = self._own_events()
            evs = (C.c_void_p * len(events))(*[e.cuda_event for e in events])
        try:
            if Program.timing_log is not None:  # bench.py's in-situ pass: every launch of this run bracketed by two timing events
                self._run_timed(L, streams, evs)
            else:
                cabi.check(L.i2r_run_program(self._c_ops, len(self.ops), streams, evs), "i2r_run_program")
        except Exception:
            # a launch list that stopped half-way may leave hand-off counters of the encoder's partial key split non-zero; the
            # kernels rely on finding them zero (include/i2r_hip.h: split_cnt)
            for t in self.split_counters:
                t.zero_()
            raise

    # In-situ per-launch timing (bench.py `roofline`): while `Program.timing_log` is a list, every run() of every program
    # goes through i2r_run_program_timed and appends (program, t0 events, t1 events, the four lanes' stream handles); the forward itself --
    # streams, lanes, sibling part-batch programs, fork / join / record / wait -- is exactly the product's.  Every launch gets a STOP event bound
    # to its dispatch and (timing_markers) a START marker in front of it: elapsed(start, stop) is the kernel's own duration, whatever the
    # host or the other lanes do; the marker costs its stream ~5 us per launch (tools/probe/event_timing.hip), so the timed forward is
    # 10-20 % slower than the real one.  Without markers (only the first launch on each stream of a program has one) a launch's start is
    # the completion of what it waited for -- its predecessor on the stream, or the lanes a fork / join / wait named -- which
    # bench.in_situ_timing reconstructs from the stop events; measured on MI355X that form counts every moment a stream waits for the
    # HOST as kernel time (w48: 52.4 us per Winograd launch against 46.9 with markers) and still slows the forward by 12 %.
    # The caller synchronises, then reads the events (before the next timed run of the same program re-binds them).
    timing_log = None
    timing_markers = True  # True: a start marker in front of EVERY launch (durations = the kernels' own); False: only at stream heads

    def _run_timed(self, L, streams, evs):
        n = len(self.ops)
        key = (tuple(streams), Program.timing_markers)
        if self._tev is None or self._tev[0] != key:  # events are created once per program (lane layout, marker mode)
            t0, t1, seen = [None] * n, [None] * n, set()
            for i, (kind, lane, st) in enumerate(self.ops):
                if kind in cabi.SYNC_OPS:
                    continue
                t1[i] = torch.cuda.Event(enable_timing=True)
                t1[i].record()  # (creates the underlying hipEvent_t; the library re-binds it to the launch)
                if Program.timing_markers or streams[lane] not in seen:
                    seen.add(streams[lane])
                    t0[i] = torch.cuda.Event(enable_timing=True)
                    t0[i].record()
            torch.cuda.synchronize(self.device)
            self._tev = (key, t0, t1, (C.c_void_p * n)(*[e.cuda_event if e is not None else None for e in t0]),
                         (C.c_void_p * n)(*[e.cuda_event if e is not None else None for e in t1]))
        _, t0, t1, a0, a1 = self._tev
        cabi.check(L.i2r_run_program_timed(self._c_ops, n, streams, evs, a0, a1), "i2r_run_program_timed")
        Program.timing_log.append((self, t0, t1, key[0]))

    def _lane_flags(self):
        if self._flags is None:
            self._flags = torch.zeros(64, dtype=torch.int32, device=self.device)
        return self._flags

    def sync_timed_out(self):
        """True if a device-side wait of this program ever gave up (50 ms): its results are then not ordered and must not be used"""
        return self._flags is not None and bool(self._flags[63].item())

    def _own_events(self):
        if self._events is None:
            self._events = [torch.cuda.Event(enable_timing=False) for _ in range(16)]  # 0..7: fork / join (rotating), 8..15: record slots
            for e in self._events:
                e.record()  # forces creation of the underlying hipEvent_t
        return self._events


# ------------------------------------------------------------------------------------------------
# network assembly
# ------------------------------------------------------------------------------------------------
class _PendingFuse:
    """a fuse output whose closing pass y = ReLU((base + up(t_a)) + up(t_b)) has not been emitted: the next module's first Winograd conv
    folds it into its staging (Program.conv(fuse_in=...)); anything else closes it with Program.fuse_up_add (HRNetW48._close)"""
    __slots__ = ("base", "terms")

    def __init__(self, base, terms):
        self.base, self.terms = base, terms


class HRNetW48:
    """Packed HRNet-W48-S tower (reference interformer_pureMulti.py:675-699) + its program emitter."""

    def __init__(self, pk, p, extra):
        self.extra = extra
        s2, s3 = extra["STAGE2"], extra["STAGE3"]
        self.stride = 4 * 2 ** (s3["NUM_BRANCHES"] - 1)  # input pixels per pixel of the lowest branch, the one `reduce` reads (interformer_pureMulti.py:702)
        self.stem1 = pk.stem(p + "conv1", p + "bn1")
        self.conv2 = pk.conv(p + "conv2", p + "bn2", stride=2)
        self.layer1 = pk.bottlenecks(p + "layer1", 4)
        self.t1 = [pk.conv(p + "transition1.0.0", p + "transition1.0.1"),
                   pk.conv(p + "transition1.1.0.0", p + "transition1.1.0.1", stride=2)]
        self.stage2 = [self._module(pk, "%sstage2.%d" % (p, m), s2) for m in range(s2["NUM_MODULES"])]
        self.t2 = pk.conv(p + "transition2.2.0.0", p + "transition2.2.0.1", stride=2)
        self.stage3 = [self._module(pk, "%sstage3.%d" % (p, m), s3) for m in range(s3["NUM_MODULES"])]

    @staticmethod
    def _module(pk, q, st):
        nb = st["NUM_BRANCHES"]
        mod = dict(nb=nb, blocks=[], fuse={})
        for i in range(nb):
            mod["blocks"].append([(pk.conv("%s.branches.%d.%d.conv1" % (q, i, b), "%s.branches.%d.%d.bn1" % (q, i, b)),
                                   pk.conv("%s.branches.%d.%d.conv2" % (q, i, b), "%s.branches.%d.%d.bn2" % (q, i, b)))
                                  for b in range(st["NUM_BLOCKS"][i])])
        for i in range(nb):
            for j in range(nb):
                if j > i:
                    mod["fuse"][(i, j)] = pk.conv("%s.fuse_layers.%d.%d.0" % (q, i, j), "%s.fuse_layers.%d.%d.1" % (q, i, j))
                elif j < i:
                    mod["fuse"][(i, j)] = [pk.conv("%s.fuse_layers.%d.%d.%d.0" % (q, i, j, k),
                                                   "%s.fuse_layers.%d.%d.%d.1" % (q, i, j, k), stride=2)
                                           for k in range(i - j)]
        return mod

    @staticmethod
    def _close(P, x):
        """the closing pass of a deferred fuse output as a launch of its own"""
        if not isinstance(x, _PendingFuse):
            return x
        y = P.alloc(x.base.n, x.base.h, x.base.w, x.base.c, x.base.dt)
        P.fuse_up_add(x.base, x.terms, y, relu=True)
        P.release(x.base, *x.terms)
        return y

    @staticmethod
    def _emit_module(P, mod, xs, need=None, defer=None):
        """HighResolutionModule.forward (interformer_pureMulti.py:392-410) as grouped launches: block k of every branch
        goes out in one launch, and the fuse sums are evaluated level by level (one launch per dependency depth).
        xs may hold deferred closing passes of the module before (_PendingFuse): the first block's conv1 folds them in.
        need: indices of the outputs somebody reads (None = all); the fuse terms and closing passes of the others are not emitted and
        their entries of the result are None.  defer: per output, the PackedConv that will read it first (or None): where that conv
        can fold the closing pass (Program.fuse_in_ok) the output is returned as a _PendingFuse."""
        nb = mod["nb"]
        xs = list(xs)
        need = set(range(nb)) if need is None else {i % nb for i in need}
        for k in range(max(len(b) for b in mod["blocks"])):
            grp, ts, folded = [], {}, []
            for i in range(nb):
                if k < len(mod["blocks"][i]):
                    if isinstance(xs[i], _PendingFuse):
                        pf = xs[i]
                        xs[i] = P.alloc(pf.base.n, pf.base.h, pf.base.w, pf.base.c, pf.base.dt)  # (its own buffer: the kernel's halo reads race with in-place stores)
                        ts[i] = P.conv(pf.base, mod["blocks"][i][k][0], relu=True, group=grp, fuse_in=(pf.terms, xs[i]))
                        folded.append(pf)
                        continue
                    ts[i] = P.conv(xs[i], mod["blocks"][i][k][0], relu=True, group=grp)
            P.flush_group(grp)
            for pf in folded:
                P.release(pf.base, *pf.terms)
            for i, t in ts.items():
                y = P.conv(t, mod["blocks"][i][k][1], relu=True, res1=xs[i], group=grp)
                P.release(t, xs[i])
                xs[i] = y
            P.flush_group(grp)
        xs = [HRNetW48._close(P, x) for x in xs]  # (a branch without blocks)
        # fuse (interformer_pureMulti.py:392-410): y_i = ReLU(sum_j f_ij(x_j)), f_ii = identity, summed left to right.
        #  * down-sampling terms (j < i, chains of stride-2 convs) are evaluated level by level, one grouped launch per level: every
        #    chain advances one conv per level while, per output, at most one term whose source is ready is ACCUMULATED into y_i
        #    (running sum in place; the identity x_i rides as a residual of the first term).  Terms are taken shortest chain first,
        #    so a two-conv chain runs beside the other terms' sums: 2 levels for three branches.
        #  * up-sampling terms (j > i: 1x1 conv + BN, nearest up-sampling) write their small low-resolution maps t_ij in the LAST of
        #    those grouped launches (plain epilogues), and one HBM-bound closing pass per output adds them:
        #    y_i = ReLU((base + up(t_i,a)) + up(t_i,b)) (i2r_fuse_up_add), base = x_i or the down-sampling partial sum.  Before, the
        #    conv epilogues scattered s x s read-modify-writes per conv pixel (load -> add -> store, serialised per destination:
        #    those launches ran at 21 TFLOP/s).
        #  The down-sampling terms all precede the identity and the up-sampling terms in the reference's j order, so only the order
        #  WITHIN the down-sampling part differs from it (three-term sums of output 2: rounding only).
        terms, ups = [], []
        for i in range(nb):
            ts = []
            for j in range(i if i in need else 0):
                chain = mod["fuse"][(i, j)]
                ts.append(dict(j=j, mids=list(chain[:-1]), last=chain[-1], cur=None))
            ts.sort(key=lambda t: (len(t["mids"]), t["j"]))
            terms.append(ts)
            ups.append([(j, mod["fuse"][(i, j)]) for j in range(i + 1, nb)] if i in need else [])
        n_up = sum(len(u) for u in ups)
        ys = [None] * nb
        n_sum = [0] * nb
        tmaps = [[] for _ in range(nb)]
        levels_left = max([1 + len(t["mids"]) for ts in terms for t in ts] + [1 if n_up else 0])
        while levels_left > 0:
            levels_left -= 1
            grp, rel = [], []
            for i in range(nb):
                ready = [t for t in terms[i] if not t["mids"]]  # (as of the start of this level)
                for t in terms[i]:
                    if t["mids"]:
                        src = t["cur"] if t["cur"] is not None else xs[t["j"]]
                        nxt = P.conv(src, t["mids"].pop(0), relu=True, group=grp)
                        if t["cur"] is not None:
                            rel.append(t["cur"])
                        t["cur"] = nxt
                if ready:
                    t = ready[0]
                    terms[i].remove(t)
                    src = t["cur"] if t["cur"] is not None else xs[t["j"]]
                    if ys[i] is None:
                        ys[i] = P.alloc(xs[i].n, xs[i].h, xs[i].w, xs[i].c, xs[i].dt)
                    # ReLU here only if nothing else is added afterwards (no further down-sampling term, no up-sampling term)
                    P.conv(src, t["last"], relu=(not terms[i] and not ups[i]), res1=xs[i] if n_sum[i] == 0 else ys[i], out=ys[i], group=grp)
                    n_sum[i] += 1
                    if t["cur"] is not None:
                        rel.append(t["cur"])
            if levels_left == 0 and n_up:  # the 1x1 convs of the up-sampling terms: small maps, plain epilogues
                cands = [(i, j, pc) for i in range(nb) for j, pc in ups[i]]
                if len(grp) + len(cands) > cabi.MAX_GROUP:  # (too many members for one launch: the 1x1 convs go out on their own)
                    P.flush_group(grp)
                for i, j, pc in cands:
                    tmaps[i].append(P.conv(xs[j], pc, group=grp))
                    if len(grp) == cabi.MAX_GROUP:
                        P.flush_group(grp)
            P.flush_group(grp)
            P.release(*rel)
        assert not any(terms)
        kept = []  # inputs that live on as the base of a deferred closing pass
        for i in range(nb):
            if not tmaps[i]:
                continue
            base = xs[i] if ys[i] is None else ys[i]
            if FUSE_IN and defer is not None and defer[i] is not None and P.fuse_in_ok(base, tmaps[i], defer[i]):
                if ys[i] is None:
                    kept.append(xs[i])
                ys[i] = _PendingFuse(base, list(tmaps[i]))
                continue
            if ys[i] is None:
                ys[i] = P.alloc(xs[i].n, xs[i].h, xs[i].w, xs[i].c, xs[i].dt)
            pend = list(tmaps[i])
            while pend:  # (two terms per pass; HRNet-W48-S has at most two lower branches)
                now, pend = pend[:2], pend[2:]
                P.fuse_up_add(base, now, ys[i], relu=not pend)
                base = ys[i]
            P.release(*tmaps[i])
        P.release(*[x for x in xs if not any(x is k for k in kept)])
        return ys

    def emit(self, P, n, h, w, n_src=None, need=None):
        """-> (list of branch Acts, stem StemArgs to patch the input pointer into).  need: indices of the branch outputs the caller reads
        (None = all): the last module then skips the fuse sums of the others, whose entries come back as None."""
        a, stem_args = P.stem(self.stem1, n, h, w, n_src=n_src, out_dt=P.store_dt)  # 16-bit modes: the whole tower stores 16 bit
        x = P.stem_conv2_layer1(a, self.conv2, self.layer1)
        grp = []  # the two transition convs read the same map: one grouped launch (304 -> 281 us at 32 crops, tools/group_try.py)
        xs = [P.conv(x, self.t1[0], relu=True, group=grp), P.conv(x, self.t1[1], relu=True, group=grp)]
        P.flush_group(grp)
        P.release(x)
        if not PRUNE_FUSE:
            need = None
        # a module's closing passes are deferred to the first block convs of the module after it (branch i reads output i)
        mods = list(self.stage2) + list(self.stage3)
        def first_convs(m, nb):
            nxt = mods[m + 1]["blocks"] if m + 1 < len(mods) else []
            return [nxt[i][0][0] if i < len(nxt) and nxt[i] else None for i in range(nb)]
        for m, mod in enumerate(self.stage2):
            xs = self._emit_module(P, mod, xs, defer=first_convs(m, mod["nb"]))
        xs[-1] = self._close(P, xs[-1])  # (the lowest branch has no up-sampling terms, so nothing is pending here today)
        t = P.conv(xs[-1], self.t2, relu=True)
        xs = [xs[0], xs[1], t]
        for m, mod in enumerate(self.stage3, len(self.stage2)):
            last = m + 1 == len(mods)
            xs = self._emit_module(P, mod, xs, need=need if last else None, defer=None if last else first_convs(m, mod["nb"]))
        return xs, stem_args


class HRFormerB:
    """Packed HRFormer-B tower (reference hrformer.py:2057-2092, arch :2489-2525) + program emitter."""

    def __init__(self, pk, p):
        from .arch_hrformer import STAGES
        b = p + "backbone."
        self.stem1 = pk.stem(b + "conv1", b + "bn1")
        self.conv2 = pk.conv(b + "conv2", b + "bn2", stride=2)
        self.layer1 = pk.bottlenecks(b + "layer1", 2)
        self.stages = []
        pre = [256]
        for sname, tname in (("stage2", "transition1"), ("stage3", "transition2"), ("stage4", "transition3")):
            st = STAGES[sname]
            ch = st["num_channels"]
            trans = []
            for i in range(st["num_branches"]):
                if i < len(pre):
                    trans.append(pk.conv("%s%s.%d.0" % (b, tname, i), "%s%s.%d.1" % (b, tname, i)) if ch[i] != pre[i] else None)
                else:
                    trans.append(pk.conv("%s%s.%d.0.0" % (b, tname, i), "%s%s.%d.0.1" % (b, tname, i), stride=2))
            mods = []
            for m in range(st["num_modules"]):
                multiscale = not (sname == "stage4" and m == st["num_modules"] - 1)
                mods.append(self._module(pk, "%s%s.%d" % (b, sname, m), st, multiscale))
            self.stages.append(dict(trans=trans, mods=mods, n_pre=len(pre)))
            pre = list(ch)

    @staticmethod
    def _module(pk, q, st, multiscale):
        nb, ch = st["num_branches"], st["num_channels"]
        mod = dict(nb=nb, n_out=nb if multiscale else 1, blocks=[], fuse={})
        for i in range(nb):
            blks = []
            for k in range(st["num_blocks"][i]):
                r = "%s.branches.%d.%d" % (q, i, k)
                fused = pk.attn_block_lp(r, ch[i], st["num_heads"][i]) if (pk.dtype != 0 and ch[i] in _HRT_FUSED_ATTN) else None
                fused_mlp = pk.mlp_block_lp(r, ch[i]) if (pk.dtype != 0 and ch[i] in _HRT_FUSED_MLP) else None
                blks.append(dict(c=ch[i], heads=st["num_heads"][i], ln1=pk.ln(r + ".norm1", ch[i]), ln2=pk.ln(r + ".norm2", ch[i]), attn_lp=fused, mlp_lp=fused_mlp,
                                 qkv=pk.qkv(r + ".attn.attn", ch[i], st["num_heads"][i]),
                                 out=pk.attn_out(r + ".attn.attn", ch[i], st["num_heads"][i]),
                                 fc1=pk.conv(r + ".mlp.fc1", r + ".mlp.norm1"), dw=pk.dw(r + ".mlp.dw3x3", r + ".mlp.norm2"),
                                 fc2=pk.conv(r + ".mlp.fc2", r + ".mlp.norm3")))
            mod["blocks"].append(blks)
        for i in range(mod["n_out"]):
            for j in range(nb):
                r = "%s.fuse_layers.%d.%d" % (q, i, j)
                if j > i:
                    mod["fuse"][(i, j)] = pk.conv(r + ".0", r + ".1")
                elif j < i:
                    mod["fuse"][(i, j)] = [(pk.dw("%s.%d.0" % (r, k), "%s.%d.1" % (r, k)), pk.conv("%s.%d.2" % (r, k), "%s.%d.3" % (r, k)))
                                           for k in range(i - j)]
        return mod

    @staticmethod
    def _emit_block(P, blk, x, lane=0):
        """GeneralTransformerBlock.forward (hrformer.py:1230-1240): x += attn(LN1 x); x += mlp(LN2 x)."""
        P.lane_ctx = lane
        if blk.get("attn_lp") is not None:  # 16-bit modes, high-resolution branches: the whole attention half in one launch
            x1 = P.hrt_attn(x, blk["attn_lp"], lane=lane)
            P.release(x)
        else:
            n1 = P.layernorm(x, blk["ln1"], lane=lane, out_dt=P.store_dt)
            qkv = P.conv(n1, blk["qkv"], lane=lane, out_dt=0)
            P.release(n1)
            a = P.winattn(qkv, blk["qkv"].bias, blk["c"], blk["heads"], lane=lane)
            P.release(qkv)
            x1 = P.conv(a, blk["out"], res1=x, lane=lane)
            P.release(a, x)
        if blk.get("mlp_lp") is not None:  # 16-bit modes, high-resolution branches: the whole MLP half in one launch
            x2 = P.hrt_mlp(x1, blk["mlp_lp"], lane=lane)
            P.release(x1)
            return x2
        # 16-bit modes: LN2's output and the 4C-wide hidden tensor of the MLP (the largest maps of the block) are stored in 16 bit;
        # the residual stream x stays fp32
        n2 = P.layernorm(x1, blk["ln2"], lane=lane, out_dt=P.store_dt)
        h1 = P.conv(n2, blk["fc1"], act=2, lane=lane)           # (keeps n2's storage type)
        P.release(n2)
        h2 = P.dwconv(h1, blk["dw"], 1, act=2, lane=lane)
        P.release(h1)
        x2 = P.conv(h2, blk["fc2"], act=2, res_post=x1, lane=lane, out_dt=0)
        P.release(h2, x1)
        return x2

    @classmethod
    def _emit_module(cls, P, mod, xs, lanes):
        """One HighResolutionTransformerModule.  With `lanes` the caller has forked lanes 0..nb-1 for the whole STAGE: branch i and fuse
        output i both run on lane i, so the only synchronisation of a module is one round of point-to-point records and waits between
        its branch blocks and its fuse layers (every output reads every branch, hrformer.py:1716-1731) -- the next module's blocks of
        branch i read what lane i itself has just written."""
        nb = mod["nb"]
        xs = list(xs)
        # The branches of a module are independent until the fuse layers (hrformer.py:1708-1715) and the low-resolution ones are far
        # too small to fill 256 CUs on their own (16x12: 160 workgroups): launches are emitted round-robin over the branches so every
        # lane's queue fills from the start.
        for k in range(max(len(b) for b in mod["blocks"])):
            for i in range(nb):
                if k < len(mod["blocks"][i]):
                    xs[i] = cls._emit_block(P, mod["blocks"][i][k], xs[i], lane=i if lanes else 0)
        # Down paths of the fuse layers (output i > source j: hops of dw 3x3 s2 + 1x1 conv, hrformer.py:1656-1700) read only branch j
        # until their last 1x1 conv, which adds the running sum of output i.  Everything before that conv runs on lane j BEFORE the
        # records: the high-resolution lanes finish their blocks early (fused kernels) while the low-resolution lanes, with
        # eight small launches per block, are the longest of every region (tools/op_list.py) -- and would otherwise also run the
        # down paths' dw convs over the big maps.
        pre, pre_y = {}, {}
        if lanes:
            for i in range(mod["n_out"]):
                for j in range(i):
                    P.lane_ctx = j
                    cur = xs[j]
                    hops = mod["fuse"][(i, j)]
                    for k, (dw, pc) in enumerate(hops):
                        d = P.dwconv(cur, dw, 2, act=0, lane=j)
                        if cur is not xs[j]:
                            P.release(cur)
                        if k < len(hops) - 1:
                            cur = P.conv(d, pc, relu=True, lane=j)
                            P.release(d)
                    pre[(i, j)] = d
                    if j == 0 and i >= 2:
                        # the FIRST term of output i >= 2 adds nothing (y = fuse[i][0](x_0), hrformer.py:1718): its last 1x1 conv runs here
                        # too, on the source lane -- the low-resolution lane i, the last to finish its blocks, then has one launch less
                        # between its blocks and the next module's
                        y0 = P.alloc(xs[i].n, xs[i].h, xs[i].w, xs[i].c)
                        P.conv(d, hops[-1][1], relu=False, out=y0, lane=j)
                        P.release(d)
                        pre_y[i] = y0
        # Point-to-point waits (round 6): every lane records behind its blocks (and the down-path prologues); a fuse lane waits for lane j
        # right before its first launch that reads lane j's data.  The low-resolution lane is the last to finish its blocks, and the terms
        # that do not read it -- the 1x1 convs over the other branches, the last convs of the down paths -- run under it instead of ~20 us
        # after it (an all-to-all barrier, rounds 3-5).
        slots, waited = {}, {}
        if lanes:
            slots = P.records(range(nb))
            waited = {l: {l} for l in range(nb)}

        def need(ln, j):  # lane ln is about to read what branch j's lane wrote before the records
            if lanes and j not in waited[ln]:
                P.wait(ln, slots[j])
                waited[ln].add(j)
        outs = []
        for i in range(mod["n_out"]):
            ln = i if lanes else 0
            P.lane_ctx = ln
            # y = ((t_0 + t_1) + ...) then ReLU (hrformer.py:1716-1731); identity terms ride as residual inputs
            acc, y, j = None, None, 0
            while j < nb:
                if j == i:
                    assert acc is None
                    acc = xs[i]
                    j += 1
                    continue
                if j == 0 and i in pre_y:  # (the whole first term ran on lane 0 ahead of the records)
                    need(ln, 0)
                    acc, y, j = pre_y[i], pre_y[i], 1
                    continue
                if y is None:
                    y = P.alloc(xs[i].n, xs[i].h, xs[i].w, xs[i].c)
                if j > i:  # 1x1 conv + BN at low resolution of EVERY lower branch (they are the trailing terms of the sum), then
                    # ONE pass that up-samples and adds them in order, + ReLU (bit-identical to a pass per term)
                    ts = []
                    for jj in range(j, nb):
                        need(ln, jj)
                        ts.append(P.conv(xs[jj], mod["fuse"][(i, jj)], lane=ln))
                    for k0 in range(0, len(ts), 3):
                        P.upsample_add(ts[k0:k0 + 3], acc if k0 == 0 else y, y, act=1 if k0 + 3 >= len(ts) else 0, lane=ln)
                    P.release(*ts)
                    jn = nb
                else:
                    cur = xs[j]
                    hops = mod["fuse"][(i, j)]
                    need(ln, j)
                    for k, (dw, pc) in enumerate(hops):
                        if (i, j) in pre:  # (everything up to the last dw conv ran on lane j before the records)
                            if k < len(hops) - 1:
                                continue
                            d = pre[(i, j)]
                        else:
                            d = P.dwconv(cur, dw, 2, act=0, lane=ln)
                            if cur is not xs[j]:
                                P.release(cur)
                        if k < len(hops) - 1:
                            cur = P.conv(d, pc, relu=True, lane=ln)
                            P.release(d)
                        else:
                            res = [acc] if acc is not None else []
                            if j + 1 == i:
                                res.append(xs[i])
                            jn = j + 2 if j + 1 == i else j + 1
                            P.conv(d, pc, relu=(jn >= nb), res1=res[0] if res else None, res2=res[1] if len(res) > 1 else None, out=y,
                                   lane=ln)
                            P.release(d)
                acc, j = y, jn
            outs.append(y)
        if lanes:  # every lane behind every record before anything released ahead of the records changes hands
            for ln in waited:
                for lj in waited:
                    if lj not in waited[ln]:
                        P.wait(ln, slots[lj])
            P.all_waited()
        P.release_deferred(*xs)  # (read by every fuse lane: reusable after the next round of waits / the stage's join)
        return outs

    def emit(self, P, n, h, w, n_src=None):
        # 16-bit modes: stem and layer1 (the 64- / 256-channel maps at 1/4 resolution, the largest of the forward) store 16 bit like the
        # HRNet tower; the transition convs hand the transformer blocks their fp32 residual stream
        a, stem_args = P.stem(self.stem1, n, h, w, n_src=n_src, out_dt=P.store_dt)
        x = P.stem_conv2_layer1(a, self.conv2, self.layer1)
        ys = [x]
        for st in self.stages:
            xs, grp = [], []  # the transition convs of a stage are independent: one grouped launch when their blocking agrees
            for i, pc in enumerate(st["trans"]):
                if i < st["n_pre"]:
                    xs.append(P.conv(ys[i], pc, relu=True, group=grp, out_dt=0) if pc is not None else ys[i])
                else:
                    xs.append(P.conv(ys[-1], pc, relu=True, group=grp, out_dt=0))
            P.flush_group(grp)
            for i, pc in enumerate(st["trans"]):  # inputs replaced by a transition conv are dead now
                if i < st["n_pre"] and pc is not None and not any(ys[i] is x_ for x_ in xs):
                    P.release(ys[i])
            # one fork region per stage: lanes 1..nb-1 start behind the transition convs (lane 0) and are joined after the last module
            nb = st["mods"][0]["nb"]
            lanes = 1 < nb <= 4
            mask = ((1 << nb) - 1) & ~1
            if lanes:
                P.fork(mask)
            for mod in st["mods"]:
                xs = self._emit_module(P, mod, xs, lanes)
            if lanes:
                P.join(mask)
            ys = xs
        return ys, stem_args


def validate_config(cfg, name=None):
    """Everything the engine refuses, checked without a GPU (Engine.__init__ runs it first; tests/test_host.py runs it over all ten
    reference experiments/*.yaml).  Raises NotImplementedError for a combination the reference can express but no shipped yaml uses."""
    M = cfg["MODEL"]
    name = name or M["NAME"]
    if name not in ("hrnet", "hrformer"):  # (every other model builds DETR-style encoder layers from these two keys)
        heads, d = M["N_HEAD"], M["DIM_MODEL"]
        if heads < 1 or d % heads:  # (nn.MultiheadAttention asserts the same)
            raise ValueError("MODEL.DIM_MODEL=%r must be divisible by MODEL.N_HEAD=%r" % (d, heads))
        if _m16(d // heads) > 256:
            raise NotImplementedError("head dim %d > 256 (i2r_mh_attention)" % (d // heads,))
    if name not in ("hrnet", "transpose_h", "hrformer", "interformer_pureMulti", "interformer", "interformer_2stage"):
        raise NotImplementedError("MODEL.NAME=%r" % (name,))
    if name in ("hrnet", "transpose_h", "hrformer"):
        return
    if M["USE_MULTI_POS"] and M["MULTI_POS_EMBEDDING"] not in ("conv", "res", "cat_vec", "sine"):
        raise NotImplementedError("MULTI_POS_EMBEDDING=%r" % (M["MULTI_POS_EMBEDDING"],))
    if M["USE_MULTI_POS"] and M["MULTI_POS_EMBEDDING"] == "sine" and (name != "interformer" or M["DIM_MODEL"] % 4):
        # PositionEmbeddingImage.forward returns a 3-D table for 'sine' (position_embedding.py:88-91): interformer_pureMulti.flatten_input
        # and interformer_2stage.flatten_input permute it as five dimensions and raise; interformer's encoder passes it through
        # (attention.py:131-137).  The sin / cos halves only stack when DIM_MODEL / 2 is even (:53-56).
        raise NotImplementedError("MULTI_POS_EMBEDDING sine with USE_MULTI_POS: the reference's own forward raises for MODEL.NAME %s / DIM_MODEL %d"
                                  % (name, M["DIM_MODEL"]))
    if M["USE_MULTI_POS"] and M["MULTI_POS_EMBEDDING"] == "cat_vec" and name == "interformer":
        wide = M["DIM_MODEL"] + M["MULTI_POS_EMBEDDING_DIM"]
        if wide % M["N_HEAD"]:
            raise ValueError("cat_vec: DIM_MODEL + MULTI_POS_EMBEDDING_DIM = %d must be divisible by N_HEAD=%r" % (wide, M["N_HEAD"]))
    if name != "interformer_pureMulti":
        sf = M["SINGLEFORMER"]
        if sf not in ("transpose_h", "hrformer") and sf:
            raise NotImplementedError("MODEL.SINGLEFORMER=%r" % (sf,))
        if not sf and name != "interformer":
            raise NotImplementedError("interformer_2stage always has a first stage")
        if sf == "hrformer" and M["DIM_MODEL"] != 78:
            raise NotImplementedError("HRFormer-B emits 78 channels (hrformer.py:2527), DIM_MODEL=%r" % (M["DIM_MODEL"],))
        if M["UPSAMPLE_TYPE"] not in ("deconv", "multiplex", "upconv"):
            raise NotImplementedError("UPSAMPLE_TYPE=%r" % (M["UPSAMPLE_TYPE"],))
        # (only interformer.py:160 reads ATTENTION_TYPE, through attention.get_encoder; interformer_2stage builds its own encoder classes)
        if name == "interformer" and M["ATTENTION_TYPE"] != "default" and M["USE_MULTI_POS"] and M["MULTI_POS_EMBEDDING"] not in ("conv", "res"):
            raise NotImplementedError("ATTENTION_TYPE=%r with MULTI_POS_EMBEDDING=%r" % (M["ATTENTION_TYPE"], M["MULTI_POS_EMBEDDING"]))
    if M["EXTRA"]["FINAL_CONV_KERNEL"] not in (1, 3):  # (the reference pads only the 3x3 case: any other size changes the map size)
        raise NotImplementedError("FINAL_CONV_KERNEL=%r (1 or 3)" % (M["EXTRA"]["FINAL_CONV_KERNEL"],))


_LANE_STREAMS = {}  # device -> side streams shared by every Engine of the process
_LANE_SPARE = {}    # device -> probed streams that share a hardware queue with the caller's stream or with a lane (kept alive, unused)
_LANE_PROBE = {}    # device -> [one record per candidate stream: what the probe measured and what became of it] (bench.py prints it as `lanes`)


def _spin_pair_ms(a, b, both, cycles):
    """ms from the start of a spin kernel on stream a to the end of it and (both) of a second one on stream b"""
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record(a)
    b.wait_event(e0)
    with torch.cuda.stream(a):
        torch.cuda._sleep(cycles)
    if both:
        with torch.cuda.stream(b):
            torch.cuda._sleep(cycles)
    e1.record(b)
    a.wait_event(e1)
    e2.record(a)
    e2.synchronize()
    return e0.elapsed_time(e2)


def _streams_overlap(a, b, cycles=100000, runs=3):
    """(overlap?, ms alone, ms together): work queued on streams a and b runs side by side (different hardware queues) if a spin kernel
    on each, started together, takes about as long as one alone (median of `runs`; ~1 ms per spin on the 100 MHz ROCm clock).
    HIP maps streams onto a handful of hardware queues in creation order; two streams on one queue serialise."""
    _spin_pair_ms(a, b, True, cycles)  # (first use of a stream binds its queue)
    t1 = sorted(_spin_pair_ms(a, b, False, cycles) for _ in range(runs))[runs // 2]
    t2 = sorted(_spin_pair_ms(a, b, True, cycles) for _ in range(runs))[runs // 2]
    return t2 < 1.5 * t1, t1, t2


def lane_streams(device, n):
    """The first n side streams of the device, created once per process and shared by all engines (lanes 1..3 of the multi-lane programs;
    the part-batch forwards run their second part on lane stream 0).  HIP spreads streams over a handful of hardware queues in the order
    they are created, and work on two streams of one queue does not overlap: an engine whose lanes landed on the caller's queue ran its
    four-lane HRFormer forward 7-16 % slower, and a process that had created an RCCL communicator first (its streams shift the order)
    lost the whole part-batch overlap (w48 fp32 3.75 -> 5.09 ms per step, tools/gather_cost.py).  So every candidate stream is PROBED:
    it becomes a lane only if a spin kernel on it runs side by side with one on the current stream and on every lane chosen so far
    (_streams_overlap); candidates that share a queue are kept aside.  At most 12 candidates; every probe is recorded in _LANE_PROBE
    (bench.py: `lanes`); I2R_LANE_PROBE=0 takes the streams as they come.  A process that is going to create an RCCL communicator calls
    this BEFORE init_process_group (bench.py does), so the lanes' queues do not depend on what RCCL creates.  Engines of one process
    issue their forwards one after the other, so sharing the streams costs nothing; it only adds ordering if they ever did not."""
    key = str(device)
    lst = _LANE_STREAMS.setdefault(key, [])
    if len(lst) < n:
        probe = os.environ.get("I2R_LANE_PROBE", "1") != "0" and hasattr(torch.cuda, "_sleep")
        log = _LANE_PROBE.setdefault(key, [])
        with torch.cuda.device(device):
            cur = torch.cuda.current_stream(device)
            _LANE_CALLER.setdefault(key, cur.cuda_stream)
            spare = _LANE_SPARE.setdefault(key, [])
            tries = 0
            while len(lst) < n and tries < 12:
                tries += 1
                st = torch.cuda.Stream(device=device)
                rec = {"stream": hex(st.cuda_stream), "candidate": tries}
                ok = True
                if probe:
                    for who, other in [("caller", cur)] + [("lane%d" % (i + 1), o) for i, o in enumerate(lst)]:
                        ok, t1, t2 = _streams_overlap(other, st)
                        rec["vs_" + who] = {"alone_ms": round(t1, 3), "together_ms": round(t2, 3), "overlap": ok}
                        if not ok:
                            break
                else:
                    rec["probe"] = "off"
                rec["role"] = ("lane%d" % (len(lst) + 1)) if ok else "spare (shares a hardware queue)"
                log.append(rec)
                (lst if ok else spare).append(st)
            while len(lst) < n:  # (fewer independent queues than lanes: the remaining lanes share)
                st = spare.pop() if spare else torch.cuda.Stream(device=device)
                log.append({"stream": hex(st.cuda_stream), "role": "lane%d (no independent queue left: shares)" % (len(lst) + 1)})
                lst.append(st)
            torch.cuda.synchronize(device)
    return lst[:n]


_LANE_CALLER = {}   # device -> handle of the caller's stream the lanes were probed against


def lanes_independent(device, streams, caller=None):
    """True if every one of `streams` is a PROBED lane of the device that ran beside the caller's stream and beside every lane chosen
    before it (lane_streams recorded `overlap: true` for all its pairs) -- i.e. each has a hardware queue of its own.  Streams that were
    taken without a probe (I2R_LANE_PROBE=0, no spin kernel) or that had to share a queue do not qualify."""
    key = str(device)
    ok = {int(r["stream"], 16) for r in _LANE_PROBE.get(key, []) if str(r.get("role", "")).startswith("lane") and "shares" not in r["role"]
          and any(k.startswith("vs_") for k in r) and all(v["overlap"] for k, v in r.items() if k.startswith("vs_"))}
    if caller is not None and _LANE_CALLER.get(key) != caller:  # (probed against another caller stream: nothing is known about this one)
        return False
    return all(s.cuda_stream in ok for s in streams)


def lane_report(device):
    """what lane_streams found on this device, for the bench line"""
    key = str(torch.device(device)) if not isinstance(device, str) else device
    lst = _LANE_STREAMS.get(key, [])
    return {"lanes": [hex(s.cuda_stream) for s in lst], "candidates": list(_LANE_PROBE.get(key, [])),
            # fork / join / record / wait of the multi-lane programs as device-side signal / wait kernels (csrc/i2r_api.hip): only with
            # independent hardware queues under every lane, and only for forwards issued from the stream the lanes were probed against
            "device_side_sync": bool(DEVICE_SYNC and len(lst) >= 3 and lanes_independent(key, lst[:3])),
            "profiler_attached": PROFILER_ATTACHED}


def _multi(y):
    """the 'multi' heat maps of what a forward returned (a dict where the model supervises its first stage too)"""
    return y["multi"] if isinstance(y, dict) else y


class Engine:
    """Packed model + program cache for one device. Built by models/_base.I2RModule."""

    def __init__(self, cfg, state_dict, device, precision="fp32", name=None):
        validate_config(cfg, name)
        cabi.lib()  # fail loudly here when the HIP library is absent
        self.precision = precision
        self.store_dt = PRECISIONS[precision]  # 16-bit modes: the conv tower keeps its activations in bf16 / f16 (half the HBM traffic)
        self.cfg = cfg
        self.device = torch.device(device)
        assert self.device.type == "cuda", "the product path runs on the GPU only (device=%s)" % (device,)
        if self.device.index is None:  # a bare 'cuda' means the CURRENT device, not device 0
            self.device = torch.device("cuda", torch.cuda.current_device())
        cabi.require_gfx950(self.device.index)
        self.programs = {}
        self.n_builds = 0  # programs built so far (bench.py --ragged-stream reports them)
        self.last_programs = []   # the program(s) of the most recent forward (bench.py's per-launch timing pass replays them)
        self.last_concurrent = []  # ... those of them that ran side by side on their own streams
        self.side_streams = lane_streams(self.device, 3)
        self._part_streams, self._part_events = [], []  # streams / events of the concurrent part-batches (_fork_parts)
        M = cfg["MODEL"]
        self.name = name or M["NAME"]
        pk = Packer(state_dict, self.device, precision)
        d, dff = M["DIM_MODEL"], M["DIM_FEEDFORWARD"]
        self._pk = pk
        self._pk32 = None          # the fp32 packer of the general encoder layer and the capture packs (_fp32_packer)
        self._capture_packs = {}   # (stack, layer) -> fp32 q|k pack of a fused layer (_capture_spec)
        self._sine_tables = {}     # (n, h, w, d) -> canvas table (_sine_table)
        # what a model does not have stays None / empty: the first stage (_pack_single), the position branch (_pack_pos), the
        # inter-human stack and the up-sampling layers below
        self.tower = self.reduce = self.head = None
        self.single_stack = self.single_pos = self.single_head = self.res_layer = self.single_tokens = None
        self.single_layers, self.layers, self.deconvs = [], [], []
        self.use_pos, self.pe_mode, self.return_dict = False, None, False
        self.win_block = self.cat_fc = self.upconv = self.domain_trans = None
        self.inter_stack = "global_encoder" if self.name == "interformer_pureMulti" else "multi_global_encoder"  # state-dict prefix of the inter-human stack
        # forward_pre exists in every copy of the layer class, but only attention.py:1040 (get_default_encoder: the inter-human stack of
        # MODEL.NAME interformer) passes cfg.MODEL.NORMALIZE_BEFORE on; the other constructors leave the default False
        self.pre_norm = bool(M["NORMALIZE_BEFORE"]) and self.name == "interformer"
        # interformer.py:296-303 (and only there): 'cat_vec' CONCATENATES the per-person vector to the token channels, the inter-human
        # encoder is DIM_MODEL + MULTI_POS_EMBEDDING_DIM wide (attention.py:1035-1040) and a 1x1 conv `fc` brings the width back
        self.cat_concat = self.name == "interformer" and M["MULTI_POS_EMBEDDING"] == "cat_vec" and bool(M["USE_MULTI_POS"])
        # interformer.py:160 -> attention.get_encoder: any ATTENTION_TYPE but 'default' swaps the encoder stack for ONE GeneralTransformerBlock
        # (attention.py:991-1031): a multi-head attention over the padded person sequence whose output is re-viewed, see _build
        self.window_attn = self.name == "interformer" and M["ATTENTION_TYPE"] != "default"
        self.singleformer = None
        if self.name == "hrnet":  # stand-alone backbone (models/hrnet.py): tower + reduce, see forward_backbone()
            self.tower = HRNetW48(pk, "", M["EXTRA"])
            self.reduce = pk.conv("reduce")
        elif self.name in ("transpose_h", "hrformer"):  # stand-alone first stage (models/transpose_h.py, models/hrformer.py): forward_single()
            self.singleformer = self.name
            self._pack_single(pk, self.name, "")
        elif self.name == "interformer_pureMulti":
            self.tower = HRNetW48(pk, "", M["EXTRA"])
            self.reduce = pk.conv("reduce")
            self.use_pos = bool(M["USE_MULTI_POS"])
            if self.use_pos:
                self._pack_pos(pk, "position_embedding", M["MULTI_POS_EMBEDDING"])
            self.layers = [self._enc_layer("global_encoder.layers.%d" % l) for l in range(M["ENCODER_LAYERS"])]
            self.deconvs = [pk.deconv("deconv_layers.0", "deconv_layers.1")] * 2  # the same layer twice (:774-775)
            self.head = pk.head("final_layer")
        elif self.name in ("interformer", "interformer_2stage"):
            sf = M["SINGLEFORMER"]
            self.singleformer = sf
            if sf:
                self._pack_single(pk, sf, "singleformer.")
            elif not sf:  # bare backbone: hrnet.HRNet.forward = reduce(lowest branch) (hrnet.py:419-446), no first-stage head
                assert self.name == "interformer", "interformer_2stage always has a first stage"
                self.tower = HRNetW48(pk, "backbone.body.", M["EXTRA"])
                self.reduce = pk.conv("backbone.body.reduce")
            self.use_pos = bool(M["USE_MULTI_POS"])
            if self.use_pos:
                self._pack_pos(pk, "multi_position_embedding", M["MULTI_POS_EMBEDDING"])
            wide = d + (M["MULTI_POS_EMBEDDING_DIM"] if self.cat_concat else 0)
            if self.window_attn:
                self.win_block = self._fp32_packer().window_block("multi_global_encoder.attn.attn", d, M["N_HEAD"])
            else:
                self.layers = [self._enc_layer("multi_global_encoder.layers.%d" % l, self.pre_norm, d=wide) for l in range(M["ENCODER_MULTI_LAYERS"])]
            if self.cat_concat:
                self.cat_fc = pk.conv("fc")
            up = M["UPSAMPLE_TYPE"]
            if up == "deconv" and self.name == "interformer_2stage":  # deconv_layers1..3, as many as pooling steps (:366-379)
                w4 = M["IMAGE_SIZE"][0] // 4
                n = int(math.log(w4 // (w4 >> int(math.log(w4 // M["TRANS_SIZE"][-1], 2))), 2))
                self.deconvs = [pk.deconv("deconv_layers%d.0" % (i + 1), "deconv_layers%d.1" % (i + 1)) for i in range(n)]
            elif up == "deconv":
                n = int(math.log(M["HEATMAP_SIZE"][0] // M["TRANS_SIZE"][1], 2))
                self.deconvs = [pk.deconv("upsample_layer.deconv_layers.%d.0" % i, "upsample_layer.deconv_layers.%d.1" % i)
                                for i in range(n)]
            elif up == "multiplex":
                self.deconvs = [pk.deconv("deconv_layers.0", "deconv_layers.1")] * 2
            elif up == "upconv":
                # UpConv (interformer.py:25-64 as upsample_layer; interformer_2stage.py:174-206,244 as upsample_conv): 1x1 conv + BN, nearest
                # upsampling by HEATMAP_SIZE[0] // TRANS_SIZE[1] (the conv kernel replicates its outputs), then (3x3 conv + BN + ReLU) twice
                q = "upsample_layer" if self.name == "interformer" else "upsample_conv"
                self.upconv = dict(scale=M["HEATMAP_SIZE"][0] // M["TRANS_SIZE"][1], fuse=pk.conv(q + ".fuse_layers.0", q + ".fuse_layers.1"),
                                   c1=pk.conv(q + ".double_conv.0", q + ".double_conv.1"), c2=pk.conv(q + ".double_conv.3", q + ".double_conv.4"))
            else:
                raise NotImplementedError("UPSAMPLE_TYPE=%r" % up)
            self.head = pk.head("final_layer")
            # interformer_2stage.py:277-279,413-414: x = domain_trans_1(single_res) + domain_trans_2(x) (two 1x1 convs with bias) instead of the sum
            if self.name == "interformer_2stage" and M["DOMAIN_TRANS"]:
                self.domain_trans = (pk.conv("domain_trans_1"), pk.conv("domain_trans_2"))
            self.return_dict = bool(M["INTER_SUPERVISION"]) and not M["SINGLEFORMER_FIX"] and bool(sf)
        else:
            raise NotImplementedError("MODEL.NAME=%r" % self.name)

    def _enc_layer(self, p, pre_norm=False, d=None):
        """One encoder layer under state-dict prefix p: the fused single-head post-norm kernels (i2r_encoder_layer) for what every shipped
        yaml asks for, else the general layer around i2r_mh_attention (any N_HEAD, pre-norm, other widths), always in fp32."""
        M = self.cfg["MODEL"]
        d, dff, heads = d or M["DIM_MODEL"], M["DIM_FEEDFORWARD"], M["N_HEAD"]
        if heads == 1 and not pre_norm and _r16(d) in (96, 80) and _r16(dff) == 192:
            return self._pk.encoder_layer(p, d, dff)
        return self._fp32_packer().encoder_layer_mh(p, d, dff, heads)

    def _fp32_packer(self):
        """the packer of what always runs in fp32 (general encoder layer, window block, capture q|k): the model's own in fp32 mode"""
        if self._pk32 is None:
            self._pk32 = self._pk if self._pk.dtype == 0 else Packer(self._pk.sd, self.device, "fp32")
        return self._pk32

    def capture_stacks(self):
        """encoder stacks whose attention maps forward(..., capture=) / forward_single(..., capture=) can return: state-dict prefix ->
        number of layers (the window-type block and the HRFormer stage are not encoder stacks)"""
        out = {}
        if self.single_layers:
            out[self.single_stack] = len(self.single_layers)
        if self.layers:
            out[self.inter_stack] = len(self.layers)
        return out

    def capture_map_sizes(self, H, W):
        """token map (h, w) of every capture stack for [H, W] network inputs: stack -> (h, w); a group of that stack is persons * h * w tokens"""
        M, out = self.cfg["MODEL"], {}
        fh = fw = None
        if self.single_layers:
            r = 4 * 2 ** self.res_layer
            fh, fw = H // r, W // r
            out[self.single_stack] = (fh, fw)
        elif self.singleformer:  # (HRFormer first stage: its highest-resolution branch)
            fh, fw = H // 4, W // 4
        if self.layers:
            if fh is None:  # the bare tower's lowest branch (_build)
                fh, fw = H // self.tower.stride, W // self.tower.stride
            else:
                for _ in range(int(math.log(fw // M["TRANS_SIZE"][-1], 2))):  # (3x3 stride-2 max-pool steps down to TRANS_SIZE)
                    fh, fw = (fh + 1) // 2, (fw + 1) // 2
            out[self.inter_stack] = (fh, fw)
        return out

    def _capture_spec(self, capture, stack, layers, d=None):
        """the Program.encoder capture argument for one stack: {layer i: a pack with fp32 q|k projection weights} -- the layer's own pack
        on the general path, else an fp32 Packer.encoder_layer_mh pack of the fused layer, built on first use"""
        want = sorted(i for st, i in capture if st == stack)
        if not want:
            return None
        cache = self._capture_packs
        packs = {}
        for i in want:
            L = layers[i]
            if not L.get("mh"):
                if (stack, i) not in cache:
                    M = self.cfg["MODEL"]
                    cache[(stack, i)] = self._fp32_packer().encoder_layer_mh("%s.layers.%d" % (stack, i), L["d"] if d is None else d, M["DIM_FEEDFORWARD"], M["N_HEAD"])
                L = cache[(stack, i)]
            packs[i] = L
        return dict(stack=stack, layers=packs)

    def _pack_single(self, pk, sf, p):
        """first (intra-human) stage under key prefix p: transpose_h.TransPoseH (:418-480) or hrformer.HRFormer (:2470-2476)"""
        M = self.cfg["MODEL"]
        d, dff = M["DIM_MODEL"], M["DIM_FEEDFORWARD"]
        if sf == "transpose_h":
            self.tower = HRNetW48(pk, p, M["EXTRA"])
            self.single_stack = p + "global_encoder"
            self.res_layer = M["HRNET_RES_LAYER"]
            self.reduce = pk.conv(p + "reduce")
            w, h = M["IMAGE_SIZE"]
            self.single_tokens = (h // 2 ** self.res_layer // 4) * (w // 2 ** self.res_layer // 4)
            self.single_pos = pk.table(p + "pos_embedding", self.single_tokens, d) if M["POS_EMBEDDING"] != "none" else None
            self.single_layers = [self._enc_layer("%sglobal_encoder.layers.%d" % (p, l)) for l in range(M["ENCODER_LAYERS"])]
            self.single_head = pk.head(p + "final_layer")
        else:
            self.tower = HRFormerB(pk, p)
            self.single_head = pk.head(p + "keypoint_head.final_layer")

    def _emit_single(self, P, S, H, W, n_src, capture=()):
        """-> (first-stage feature Act [S, H/4, W/4, d], stem args): tower (+ reduce + per-crop encoder for TransPose-H, :649-655)"""
        if self.singleformer == "hrformer":
            xs, stem_args = self.tower.emit(P, S, H, W, n_src=n_src)
            return xs[0], stem_args
        xs, stem_args = self.tower.emit(P, S, H, W, n_src=n_src, need={self.res_layer})
        f = P.conv(xs[self.res_layer], self.reduce, out_dt=0)
        P.release(*xs)
        tok = f.h * f.w
        assert tok == self.single_tokens, "input size does not match MODEL.IMAGE_SIZE (pos_embedding rows)"
        cap = self._capture_spec(capture, self.single_stack, self.single_layers) if capture else None
        g = P.encoder(f, self.single_layers, [i * tok for i in range(S + 1)],
                      pos=self.single_pos.data_ptr() if self.single_pos is not None else 0, pos_period=tok, pos_table=self.single_pos, capture=cap)
        if cap is None:  # (a capture program returns the stack's input: the reduce output)
            P.release(f)
        return g, stem_args

    def _pack_pos(self, pk, p, mode):
        """PositionEmbeddingImage (position_embedding.py:6-32): the two image modes that produce a per-token embedding from the bbox
        mask.  'cat_vec' changes the encoder width (interformer.py:297-303) and 'sine' ignores the mask; no shipped yaml enables
        either together with USE_MULTI_POS."""
        self.pe_mode = mode
        if mode == "conv":
            self.pe_stem = pk.stem(p + ".conv1", p + ".bn1")
            self.pe_conv2 = pk.conv(p + ".conv2", p + ".bn2", stride=2)
        elif mode == "res":
            self.pe_res = pk.pe_res(p)
        elif mode == "sine":
            pass  # (no parameters: rows of a canvas table computed on the host exactly as the reference does, _sine_table)
        elif mode == "cat_vec":
            # nn.Linear(TRANS_SIZE[0] * TRANS_SIZE[1], vec_dim) on the pooled mask (position_embedding.py:19-23): vec_dim = DIM_MODEL in
            # interformer_pureMulti.py:465, MULTI_POS_EMBEDDING_DIM in interformer.py:155 / interformer_2stage.py
            w, b = pk.sd[p + ".fc.weight"], pk.sd[p + ".fc.bias"]
            self.pe_fc = dict(w=pk._dev(w.float()), b=pk._dev(b.float()), vec=int(w.shape[0]))
            if not self.cat_concat and self.pe_fc["vec"] != self.cfg["MODEL"]["DIM_MODEL"]:  # (the reference fails on src + pos the same way)
                raise ValueError("MULTI_POS_EMBEDDING cat_vec as an additive embedding needs MULTI_POS_EMBEDDING_DIM == DIM_MODEL (%d vs %d)"
                                 % (self.pe_fc["vec"], self.cfg["MODEL"]["DIM_MODEL"]))
        else:
            raise NotImplementedError("MULTI_POS_EMBEDDING=%r with USE_MULTI_POS" % (mode,))

    # ---- program construction ----
    def _sine_table(self, n, h, w, d, cs):
        """PositionEmbeddingImage.make_sine_position_embedding (position_embedding.py:34-61) for n = max(length) persons: a sine embedding
        over a canvas of h x (n w) cells, flattened row-major; the reference adds row l to token l of the (person, y, x)-ordered sequence
        of an image (a 3-D pos is not permuted, attention.py:131-137), so person q owns rows [q h w, (q + 1) h w).  Computed on the
        host with the reference's own sequence of torch CPU ops (it builds the table on the CPU in every forward) -> [n, h w, cs] on the device."""
        key = (n, h, w, d)
        cache = self._sine_tables
        if key not in cache:
            W = n * w
            area = torch.ones(1, h, W)
            y_embed = area.cumsum(1, dtype=torch.float32)
            x_embed = area.cumsum(2, dtype=torch.float32)
            half = d // 2
            y_embed = y_embed / (y_embed[:, -1:, :] + 1e-6) * (2 * math.pi)
            x_embed = x_embed / (x_embed[:, :, -1:] + 1e-6) * (2 * math.pi)
            dim_t = torch.arange(half, dtype=torch.float32)
            dim_t = 10000 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / half)
            pos_x = x_embed[:, :, :, None] / dim_t
            pos_y = y_embed[:, :, :, None] / dim_t
            pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
            pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
            tab = torch.cat((pos_y, pos_x), dim=3).reshape(h * W, d)  # (row-major canvas)
            out = torch.zeros(n, h * w, cs)
            out[:, :, :d] = tab.view(n, h * w, d)
            if len(cache) > 16:
                cache.clear()
            cache[key] = out.to(self.device)
        return cache[key]

    def _fill_sine(self, patch, glen, sine_n):
        """rows of the 'sine' multi-position embedding for the crops of this forward (glen: persons per token group, capacity groups
        included; sine_n: max(length) of the WHOLE batch -- the canvas is that many persons wide for every part of it)"""
        pos = patch.get("pos_sine")
        if pos is None:
            return
        n = max(sine_n, 1)
        key = (n, tuple(glen))
        if patch.get("_sine_key") == key:
            return
        tab = self._sine_table(n, pos.h, pos.w, pos.c, pos.cs)
        idx = torch.tensor([q for g in glen for q in range(g)], dtype=torch.long).to(self.device, non_blocking=True)
        assert idx.numel() == pos.n
        pos.view().view(pos.n, pos.h * pos.w, pos.cs).copy_(tab[idx])
        patch["_sine_key"] = key

    def _pos_branch(self, P, n, h, w, trans_w, n_src=None, cat=None):
        """cat (mode cat_vec of MODEL.NAME interformer): the token buffer whose channels behind DIM_MODEL receive the embedding"""
        if self.pe_mode == "cat_vec":
            th = h // (w // trans_w)
            out = cat if cat is not None else P.alloc(n, th, trans_w, self.pe_fc["vec"])
            return out, P.pe_cat_vec(self.pe_fc, n, h, w, th, trans_w, out, self.cfg["MODEL"]["DIM_MODEL"] if cat is not None else 0, n_src=n_src)
        if self.pe_mode == "res":  # conv_pre -> resnet18[:5] -> conv_end (position_embedding.py:93-97), then the pooling loop (:106-109)
            r = self.pe_res
            a, pe_args = P.pe_res_stem(r, n, h, w, n_src=n_src)
            b = P.maxpool(a)
            P.release(a)
            for c1, c2 in r["blocks"]:  # torchvision BasicBlock: conv-bn-relu-conv-bn, + identity, relu
                t = P.conv(b, c1, relu=True)
                y = P.conv(t, c2, relu=True, res1=b)
                P.release(t, b)
                b = y
            a = b
            b = P.conv(a, r["conv_end"])
            P.release(a)
        else:
            a, pe_args = P.stem(self.pe_stem, n, h, w, n_src=n_src)
            b = P.conv(a, self.pe_conv2, relu=True)
            P.release(a)
        for _ in range(int(math.log(b.w // trans_w, 2))):
            c = P.maxpool(b)
            P.release(b)
            b = c
        return b, pe_args

    def _pool_to_trans(self, P, g, out=None):
        """the first-stage features g pooled down to TRANS_SIZE (3x3 stride-2 max-pool steps); g itself stays (the tail reads it).
        out: the destination of the last step (the token buffer of a channel concatenation)"""
        steps = int(math.log(g.w // self.cfg["MODEL"]["TRANS_SIZE"][-1], 2))
        if out is not None and steps == 0:
            raise NotImplementedError("cat_vec with a first stage whose maps already are TRANS_SIZE")
        f = g
        for i in range(steps):
            c = P.maxpool(f, out=out if i == steps - 1 else None)
            if f is not g:
                P.release(f)
            f = c
        return f

    def _new_program(self, form=None):
        """an empty Program of this engine's storage type; form: the capture form of the call it is built for (attn_capture.resolve), or None"""
        P = Program(self.device)
        P.store_dt, P.form = self.store_dt, form
        return P

    def _build(self, S, H, W, length, flip=False, part=None, form=None):
        """flip: the flip test of validate() (lib/core/function.py:142-162) batched into the same forward -- crops S..2S-1 are
        the mirrored copies (mirroring happens inside the stem kernels), every image appears twice as a token group.
        part (models whose first stage is the bare HRNet tower): "tower" = the per-crop tower + reduce only -> (P, patch, features Act);
        "tail" = everything behind it (position branch, inter-human encoder, deconvs, head) reading a feature buffer that tower
        programs fill (patch["feat"]) -- the two halves of a part-batch forward (_forward_split).
        form: the capture form (attn_capture.resolve) -- the program computes the attention maps of form.capture too (Program.bind_capture)."""
        M = self.cfg["MODEL"]
        P = self._new_program(form)
        capture = form.capture if form else ()
        patch = {}
        n_src = S
        if flip:
            S, length = 2 * S, list(length) + list(length)
        bare = self.name == "interformer_pureMulti" or not self.singleformer
        assert part is None or bare
        cat, d = None, M["DIM_MODEL"]
        if self.cat_concat:  # torch.cat([x, multi_pos], dim=2): both producers write their channel range of ONE token buffer
            assert part is None
            tw = M["TRANS_SIZE"][-1]
            cat = P.alloc(S, H // (W // tw), tw, d + self.pe_fc["vec"])
        if bare and part == "tail":
            f = patch["feat"] = P.alloc(S, H // self.tower.stride, W // self.tower.stride, self.reduce.cout)
            f.t.zero_()  # (capacity slots nobody fills must hold finite rows)
            single_feat = None
        elif bare:
            xs, patch["x"] = self.tower.emit(P, S, H, W, n_src=n_src, need={-1})  # (only the lowest branch is read below)
            if cat is not None:
                assert (xs[-1].h, xs[-1].w) == (cat.h, cat.w), "cat_vec: the backbone output is not TRANS_SIZE"
            f = P.conv(xs[-1], self.reduce, out_dt=0, out=cat)
            P.release(*xs)
            single_feat = None
            if part == "tower":
                P.finalize()
                return P, patch, f
        else:
            g, patch["x"] = self._emit_single(P, S, H, W, n_src, capture)
            single_feat = g
            if self.return_dict:
                patch["single"] = P.head(g, self.single_head)
            f = self._pool_to_trans(P, g, out=cat)
        if self.window_attn:
            e = self._emit_window_block(P, patch, f, single_feat, S, H, W, length)
            return self._emit_tail(P, patch, e, single_feat)
        pos_ptr = 0
        if self.use_pos and self.pe_mode == "sine":
            # the mask is ignored (position_embedding.py:88-91); the rows are filled per forward (_fill_sine: they depend on max(length))
            pos = patch["pos_sine"] = P.alloc(S, f.h, f.w, f.c)
            pos.t.zero_()
            pos_ptr = pos.ptr
        elif self.use_pos:
            pos, patch["pos_mask"] = self._pos_branch(P, S, H, W, M["TRANS_SIZE"][-1], n_src=n_src, cat=cat)
            assert (pos.h, pos.w, pos.cs) == (f.h, f.w, f.cs)
            pos_ptr = pos.ptr if cat is None else 0  # (concatenated: the encoder gets no additive embedding, interformer.py:299)
        cap = self._capture_spec(capture, self.inter_stack, self.layers, d=f.c) if capture else None
        e = P.encoder(f, self.layers, self._token_offsets(length, f.h * f.w), pos=pos_ptr, regroupable=True, pre_norm=self.pre_norm, capture=cap)
        if cat is not None:  # self.fc: Conv2d(DIM_MODEL + MULTI_POS_EMBEDDING_DIM, DIM_MODEL, 1) with bias (interformer.py:157-158,302-303)
            t = P.conv(e, self.cat_fc, out_dt=0)
            P.release(e)
            e = t
        return self._emit_tail(P, patch, e, single_feat)

    def _emit_window_block(self, P, patch, f, single_feat, S, H, W, length):
        """ATTENTION_TYPE != 'default' (attention.py:991-1031): the persons of every image padded to max(length) ROWS (zero features; the
        position branch of a zero mask), q|k = (x + pos) W, v = x W, multi-head attention of all P h w rows of an image over the keys of its
        real persons, out-proj (no residual, no FFN, no norm), then the re-viewing of the [L, B, C] output and get_valid_output.
        The padded layout, hence the program, belongs to this `length` (no capacity padding, no regrouping)."""
        M, L = self.cfg["MODEL"], self.win_block
        assert sum(length) == S and f.n == S
        B, Pm, hw = len(length), max(length), f.h * f.w
        starts = [sum(length[:b]) for b in range(B)]
        pad_map = [starts[b] + q if q < length[b] else -1 for b in range(B) for q in range(Pm)]
        xp = P.rows_gather(f, pad_map)
        if f is not single_feat:
            P.release(f)
        pos_p = None
        if self.use_pos:  # crops 0..S-1: the persons' masks; crop S: the zero mask every padded person gets (interformer.py:275)
            pos, patch["pos_mask"] = self._pos_branch(P, S + 1, H, W, M["TRANS_SIZE"][-1], n_src=S + 1)
            assert (pos.h, pos.w, pos.cs) == (xp.h, xp.w, xp.cs)
            pos_p = P.rows_gather(pos, [m if m >= 0 else S for m in pad_map])
            P.release(pos)
        qk = P.conv(xp, L["qk"], in2=pos_p)
        v = P.conv(xp, L["v"])
        P.release(xp)
        if pos_p is not None:
            P.release(pos_p)
        att = P.alloc(B * Pm, f.h, f.w, L["hs"])
        goff = torch.zeros(B + 1, dtype=torch.int32, device=self.device)
        klen = torch.tensor([n * hw for n in length], dtype=torch.int32).to(self.device)
        P.keep += [goff, klen, L]
        a = cabi.MhAttnArgs(qk.ptr, v.ptr, att.ptr, goff.data_ptr(), 0, L["heads"], L["hp"], L["hs"], qk.cs, v.cs, att.cs, 0, 0, 0, klen.data_ptr())
        P.ops.append((cabi.OP_MH_ATTN, 0, a))
        P._register_stack(dict(descs=[], mh=[a], goff=goff, current=None), [b * Pm * hw for b in range(B + 1)])  # (groups = the padded images)
        P.release(qk, v)
        o = P.conv(att, L["o"])
        P.release(att)
        e = P.view_scramble(o, [b * Pm + q for b in range(B) for q in range(length[b])], B, Pm, M["DIM_MODEL"])
        P.release(o)
        return e

    def _emit_tail(self, P, patch, e, single_feat):
        """up-sampling layers (+ the 2-stage residual / DOMAIN_TRANS) and final_layer behind the inter-human encoder output e"""
        dtr, uc = self.domain_trans, self.upconv
        res_feat = single_feat if dtr is None else None
        if uc is not None:
            u = P.conv(e, uc["fuse"], up=uc["scale"])
            P.release(e)
            t = P.conv(u, uc["c1"], relu=True)
            P.release(u)
            e = P.conv(t, uc["c2"], relu=True, res_post=res_feat)  # (2-stage models: x = single_res + x behind the ReLU, interformer.py:315)
            P.release(t)
        for i, dc in enumerate(self.deconvs):
            last = i == len(self.deconvs) - 1
            # 2-stage models add the first-stage features AFTER the deconv's ReLU (x = single_res + x, interformer.py:315)
            u = P.deconv(e, dc, relu=True, res_post=res_feat if (last and res_feat is not None) else None)
            P.release(e)
            e = u
        if dtr is not None:
            t = P.conv(single_feat, dtr[0], out_dt=0)
            u = P.conv(e, dtr[1], res1=t, out_dt=0)
            P.release(e, t)
            e = u
        patch["multi"] = P.head(e, self.head)
        patch["head_in"] = e  # (never released: the arena cannot hand it to another op, forward_head_input reads it behind the run)
        P.finalize()
        return P, patch

    def forward_head_input(self, x, pos_mask, length):
        """forward() plus the tensor final_layer read: -> (heatmaps [S, J, h, w], feat [S, h, w, cs]) -- feat the fp32 NHWC input of
        P.head (channel padding kept: the model's head has the true channel count), copied out of the arena because the next forward
        overwrites it.  One program (no part-batches), the default program of that capacity; its heat maps are forward()'s whenever
        forward() runs one program too.  What a head re-fit trains on (caller.HeadFit).  ValueError: a class whose forward does not end
        in the inter-human tail, the window-type block (its program belongs to one `length`), FINAL_CONV_KERNEL 3 (the head's input is
        then a 3x3 conv's, not a per-pixel product)."""
        if self.name not in ("interformer_pureMulti", "interformer", "interformer_2stage"):
            raise ValueError("forward_head_input serves the inter-human models (MODEL.NAME %r has no such tail)" % self.name)
        if self.window_attn:
            raise ValueError("forward_head_input: not with ATTENTION_TYPE %r" % self.cfg["MODEL"]["ATTENTION_TYPE"])
        if self.head.get("conv3") is not None:
            raise ValueError("forward_head_input: FINAL_CONV_KERNEL 3 -- the head re-fit is for a 1x1 final_layer")
        assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
        S, _, H, W = x.shape
        assert S == sum(length), "sum(length)=%d != number of crops %d" % (sum(length), S)
        assert all(n >= 1 for n in length), "every image needs at least one person"
        with torch.cuda.device(self.device):
            y = self._forward_part(x, pos_mask, list(length), None, S, H, W, max(length))
            P = self.last_programs[0]
            patch = next(v[1] for v in self.programs.values() if v[0] is P)
            e = patch["head_in"]
            assert e.dt == 0
            return _multi(y), e.view()[:S].clone()

    def forward_backbone(self, x):
        """hrnet.HRNet.forward (hrnet.py:419-446): x [S,3,H,W] -> reduce(lowest branch) as an NCHW tensor [S, d, H/16, W/16]."""
        assert self.name == "hrnet" and x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
        S, _, H, W = x.shape
        x = x.to(self.device).contiguous()
        key = (S, H, W, "backbone")
        with torch.cuda.device(self.device):
            def build():
                P = self._new_program()
                xs, px = self.tower.emit(P, S, H, W, n_src=S, need={-1})
                f = P.conv(xs[-1], self.reduce, out_dt=0)
                P.release(*xs)
                P.finalize()
                return (P, px, f)
            P, px, f = self._program(key, build)
            px.in_ = x.data_ptr()
            P.run()
            # (NHWC arena buffer -> the reference's NCHW tensor: a torch view + copy, boundary plumbing only)
            return f.t.view(S, f.h, f.w, f.cs)[..., :f.c].permute(0, 3, 1, 2).contiguous()

    def forward_single(self, x, capture=None, queries=None):
        """Stand-alone first stage, as the reference's InterFormer calls it (interformer.py:288): transpose_h.TransPoseH.forward
        (:649-655) / hrformer.HRFormer.forward (:2477-2480): x [S,3,H,W] -> (features [S,d,H/4,W/4], heatmaps [S,J,H/4,W/4]).
        capture, queries: see forward(); then -> ((features, heatmaps), maps)."""
        assert self.name in ("transpose_h", "hrformer") and x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
        S, _, H, W = x.shape
        x = x.to(self.device).contiguous()
        form = attn_capture.resolve(capture, queries, None, None, self.capture_stacks(), self.inter_stack, self.window_attn)
        key = (S, H, W, "single") + (form.key if form else ())
        with torch.cuda.device(self.device):
            def build():
                P = self._new_program(form)
                g, px = self._emit_single(P, S, H, W, S, form.capture if form else ())
                hd = P.head(g, self.single_head)
                P.finalize()
                return (P, px, g, hd)
            P, px, g, hd = self._program(key, build)
            px.in_ = x.data_ptr()
            J = self.cfg["MODEL"]["NUM_JOINTS"]
            hm = torch.empty(S, J, g.h, g.w, dtype=torch.float32, device=self.device)
            hd.out = hm.data_ptr()
            views = self._bind_capture(P, form, S, [], H, W) if form else None
            P.run(self.side_streams if P.uses_lanes else None)
            # (NHWC arena buffer -> the reference's NCHW feature tensor: a torch view + copy, boundary plumbing only)
            feat = g.t.view(S, g.h, g.w, g.cs)[..., :g.c].permute(0, 3, 1, 2).contiguous()
            if form:
                return (feat, hm), self._finish_capture(P, views, S, H)
        return feat, hm

    def _bind_capture(self, P, form, S, length, H, W):
        """the capture part of a call: the real crops / images of this call (the capacity slots behind them cost nothing) on the token maps
        capture_map_sizes promises (attention_at mapped its points onto them) -> the views of Program.bind_capture"""
        sizes, glens = self.capture_map_sizes(H, W), []
        for c in P.captures:
            h, w = c.x.h, c.x.w
            if sizes.get(c.stack) != (h, w):
                raise RuntimeError("capture_map_sizes(%d, %d)[%r] = %s, but the program's stack input is %d x %d"
                                   % (H, W, c.stack, sizes.get(c.stack), h, w))
            glens.append([h * w] * S if c.stack == self.single_stack else [n * h * w for n in length])
        return P.bind_capture(glens, form.call)

    @staticmethod
    def _capture_inputs(P, S):
        """per captured stack its input features [S, c, h, w] (NCHW copies: the `reduce` output for the stacks fed by one)"""
        return {(c.stack, "input"): c.x.view()[:S, :, :, :c.x.c].permute(0, 3, 1, 2).contiguous() for c in P.captures}

    @staticmethod
    def capacity(S):
        """Crop capacity of the program that serves a batch of S crops: exact up to 8, then the next multiple of 2 (<= 32), 4 (<= 64) or 8.
        In the reference's validate() loop S = sum(length) changes with nearly every batch (persons per image vary); building a
        program costs tens of ms (arena, block maps, descriptors), so programs are built per CAPACITY and a batch runs in the
        smallest one that holds it -- the unused slots are extra single-person groups whose heat maps are dropped (<= 1 / 3 / 7 wasted
        crops, i.e. <= 11 % at any size)."""
        if S <= 8:
            return S
        step = 2 if S <= 32 else (4 if S <= 64 else 8)
        return -(-S // step) * step

    # Program cache: least-recently-used programs are dropped beyond MAX_PROGRAMS entries OR beyond MAX_PROGRAM_BYTES of arena memory
    # (each program owns ~20 MB of activations per crop; a part-batch forward keeps a tower program per stream and capacity next to the
    # tail's, and a ragged validate() stream touches one capacity per batch size: a count alone does not bound the memory).
    MAX_PROGRAMS = 48
    MAX_PROGRAM_BYTES = 32 << 30

    def forward(self, x, pos_mask, length, flip_joint_map=None, capture=None, queries=None, persons=None, joints=None, flip_maps="plain", rollout=None):
        """flip_joint_map (device int32 [J], see caller.joint_map): run the flip test in the same forward and return the merged
        'multi' heatmaps (the reference merges only outputs['multi'], function.py:137-162).
        capture: a set of (stack, layer) -- stack a state-dict prefix of capture_stacks() -- whose attention maps to return as well:
        -> (output, maps), maps[(stack, layer)] = per batch entry of that stack (image: inter-human, crop: intra-human) the [L, L] fp32
        head-averaged softmax(q k^T) (views into one buffer per call), maps[(stack, "input")] = the stack's input features [S, c, h, w].
        A capture forward is one program (no part-batches), built once per capture set; the default programs are not touched.
        queries (AttnQueries, with capture): instead of the [L, L] maps, their rows (mode 0) or columns (mode 1) at the token indices
        queries.tokens[stack] (int32 [groups, K], -1 = skip), optionally up-sampled bilinearly by queries.upsample (an int, or one per
        stack): maps[(stack, layer)] = per group a [K_g, persons, h r, w r] view.  One program per (capture set, mode, K capacity, scales) --
        K is in the key although every K-dependent field is patched per call: a caller asks with one K; new points or another grouping
        at the same capacity reuse it.
        persons (PersonMaps, with capture of layers of the inter-human stack only): instead of the [L, L] maps, their reduction per person
        -> (output, (relation, maps)): relation[(stack, layer)] = per image the [P, P] matrix, maps[(stack, layer)] = per image a
        [P, P, h r, w r] view (persons.mode 1: dependency maps, 2: affect maps, 0: no entry).  One program per (capture set, mode, scale);
        another grouping at the same capacity reuses it.  ValueError: another stack, the window-type block, the flip test, queries.
        joints (JointQueries, with capture): the query form at the joints THIS forward predicts -> (output, (joints, maxvals, maps)):
        joints [S, J, 2] = 4 x the arg-max (x, y) of every 'multi' heat map (i2r_decode's arg-max: first index, (0, 0) for a map without a
        positive value), maxvals [S, J], both on the device; maps as for queries with K = J (the inter-human stack: entry person * J + j).
        i2r_joint_tokens makes the token tables from the heat maps and the i2r_attn_query_maps launches of the captured layers run behind
        the head, on the current stream, with no copy to the host in between.  It is the one form that goes with flip_joint_map: the
        program is the flip program, the tables come from the MERGED maps, the launches cover the plain half (the first groups of each
        stack); the mirrored pass's maps are not computed.  Every captured layer holds its fp32 q|k [tokens, 2 hs] until the program ends.
        One program per (capture set, mode, J, scales).  ValueError: the window-type block, queries= or persons= too, no encoder stack.
        flip_maps: "plain" (all of the above) or "merged" -- with flip_joint_map and ONE of queries, persons, joints: the maps of the flip
        test, M = (P + P~) / 2 with P~[q, k] = P'[mu(q), mu(k)] the mirrored pass's map brought back into the plain frame (DESIGN.md
        'i2r_attn_flip_merge'), in the layouts of the un-flipped calls; output is the merged heat maps.  The program is the flip program
        with a marker in its key; every captured layer holds its fp32 q|k of BOTH halves until the program ends, and the launches run
        behind the head (attn_bind.run_merge).  ValueError: without the flip test, with the full [L, L] form, the window-type block.
        rollout (attn_capture.Rollout, with capture of a contiguous layer range lo .. hi per stack): the attention roll-out T = A_hi ... A_lo,
        A_l = (1 - alpha) I + alpha P_l, THROUGH those layers instead of the maps of each (DESIGN.md 'i2r_attn_rollout_step') -- with tokens
        -> (output, {stack: maps}), maps as for queries of ONE layer: rows T[q, :] (mode 0) or columns T[:, q] (mode 1); without tokens (the
        inter-human stack only) -> (output, ({stack: relation}, {stack: maps})) as for persons.  Every captured layer holds its fp32 q|k
        until the program ends; the chain of i2r_attn_rollout_step launches runs behind the head between two working matrices in the
        capture buffer.  One program per (capture set, kind, mode, K capacity, scales); alpha, points and grouping are per call.
        ValueError: the flip test, another form, the window-type block, a layer set with a hole."""
        assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
        S, _, H, W = x.shape
        assert S == sum(length), "sum(length)=%d != number of crops %d" % (sum(length), S)
        assert all(n >= 1 for n in length), "every image needs at least one person"
        sine_n = max(length)  # (MULTI_POS_EMBEDDING sine: the canvas is max(length) persons wide, for every part of this batch)
        form = attn_capture.resolve(capture, queries, persons, flip_joint_map, self.capture_stacks(), self.inter_stack, self.window_attn,
                                    joints, self.cfg["MODEL"]["NUM_JOINTS"], flip_maps, rollout)
        if form:
            with torch.cuda.device(self.device):
                return self._forward_part(x, pos_mask, list(length), flip_joint_map if form.behind else None, S, H, W, sine_n, form=form)
        if self.window_attn and flip_joint_map is not None:
            # the window type mixes the rows of ALL images of a call (attention.py:1025-1029): the mirrored batch must be a call of its
            # own, as in validate() (function.py:142-162), not extra token groups of this one
            with torch.cuda.device(self.device):
                x = x.to(self.device)
                pm = pos_mask.to(self.device) if pos_mask is not None else None
                a = self._forward(x, pm, list(length), None, S, H, W, sine_n)
                b = self._forward(torch.flip(x, dims=[3]), torch.flip(pm, dims=[3]) if pm is not None else None, list(length), None, S, H, W, sine_n)
                return self._flip_merge(_multi(a).contiguous(), _multi(b).contiguous(), flip_joint_map, S, H, W)
        with torch.cuda.device(self.device):  # kernels and events go to the CURRENT device: make it this engine's
            return self._forward(x, pos_mask, list(length), flip_joint_map, S, H, W, sine_n)

    def _flip_merge(self, a, b, flip_joint_map, S, H, W):
        """i2r_flip_merge on the current stream: the heat maps a [>= S, J, H/4, W/4] merged with those of the mirrored crops b"""
        J = self.cfg["MODEL"]["NUM_JOINTS"]
        merged = torch.empty(S, J, H // 4, W // 4, dtype=torch.float32, device=self.device)
        cabi.check(cabi.lib().i2r_flip_merge(a.data_ptr(), b.data_ptr(), flip_joint_map.data_ptr(), merged.data_ptr(),
                                             S, J, H // 4, W // 4, torch.cuda.current_stream(self.device).cuda_stream), "i2r_flip_merge")
        return merged

    @staticmethod
    def _token_offsets(glen, tok):
        """persons per token group -> the groups' token offsets [groups + 1] at tok tokens per person"""
        offs = [0]
        for n in glen:
            offs.append(offs[-1] + n * tok)
        return offs

    # Part-batches on separate streams (round 4).  The images of a batch are independent: `_split_bounds` cuts a batch of the HRNet /
    # TransPose-H towers into SPLIT_PARTS contiguous image groups balanced by crop count (dist.shard_bounds) and `_forward` runs one
    # program per group -- each with its own arena, keyed by a slot -- on the caller's stream and on side streams, forked and joined with
    # events.  The launches of the parts interleave on the chip: one part computes while another stages or drains.  Measured
    # (tools/host_rate.py, bench.py): config 3 bf16 4.36 -> 3.75 ms, the fp32 headline 4.17 -> 3.93 ms, TransPose-H fp32 15.2 -> 14.2 ms.
    # Not for the four-lane HRFormer-B programs (twice the launches of kernels whose time barely depends on the batch: 5.2 vs 3.8 ms).
    SPLIT_MIN_CROPS = 24
    SPLIT_MIN_PART = 8   # crops of the smallest part: a [23, 1] batch would double the launches for nothing to overlap with
    SPLIT_PARTS = 2

    def _split_bounds(self, length, H=None, W=None):
        """image index cuts [0, b1, ..., n] of the concurrent part-batches, or None (one program): every part needs >= SPLIT_MIN_PART
        crops, and the tower / tail split hands features over between programs whose map sizes must agree (H, W multiples of the
        tower's total stride; any other size takes the one-program path, which handles it)"""
        from .dist import shard_bounds
        parts = min(self.SPLIT_PARTS, len(length))
        if parts < 2 or sum(length) < self.SPLIT_MIN_CROPS or not isinstance(self.tower, HRNetW48):
            return None
        if H is not None and (H % self.tower.stride or W % self.tower.stride):
            return None
        if self.cat_concat or self.window_attn:  # (the hand-over buffer is DIM_MODEL wide; the window type re-views the WHOLE batch's output)
            return None
        bounds = shard_bounds(list(length), parts)
        if not all(bounds[i + 1] > bounds[i] for i in range(parts)):
            return None
        if min(sum(length[bounds[i]:bounds[i + 1]]) for i in range(parts)) < self.SPLIT_MIN_PART:
            return None
        return bounds

    def _forward(self, x, pos_mask, length, flip_joint_map, S, H, W, sine_n):
        bounds = self._split_bounds(length, H, W)
        if bounds is None:
            return self._forward_part(x, pos_mask, length, flip_joint_map, S, H, W, sine_n, slot=0)
        if self.name == "interformer_pureMulti" or not self.singleformer:
            return self._forward_split(x, pos_mask, length, flip_joint_map, S, H, W, sine_n, bounds)
        parts = len(bounds) - 1
        offs = [sum(length[:b]) for b in bounds]
        x = x.to(self.device).contiguous()
        pm = pos_mask.to(self.device, torch.float32).contiguous() if pos_mask is not None else None
        progs = [None] * parts

        def run_part(i):
            y = self._forward_part(x[offs[i]:offs[i + 1]], pm[offs[i]:offs[i + 1]] if pm is not None else None,
                                   length[bounds[i]:bounds[i + 1]], flip_joint_map, offs[i + 1] - offs[i], H, W, sine_n, slot=i)
            progs[i] = self.last_programs
            return y
        ys = self._fork_parts(range(1, parts), [x] if pm is None else [x, pm], run_part)
        self.last_programs = [P for part in progs for P in part]
        self.last_concurrent = list(self.last_programs)
        cur = torch.cuda.current_stream(self.device)
        for y in ys[1:]:
            for t in (y.values() if isinstance(y, dict) else (y,)):
                t.record_stream(cur)  # (allocated on the side stream, consumed on the caller's)
        if isinstance(ys[0], dict):
            return {key: torch.cat([y[key] for y in ys], 0) for key in ys[0]}
        return torch.cat(ys, 0)

    def _fork_parts(self, side, inputs, run_part):
        """The fork / join of a part-batch forward.  run_part(i) issues part i on the current stream: first every side part i of `side`, in
        that order, on its own stream behind an event that marks `inputs` ready on the caller's stream, then part 0 on the caller's
        stream (its launches queue behind the side streams'), which finally waits for every side part.  -> [run_part(i)] by part."""
        parts = len(side) + 1
        cur = torch.cuda.current_stream(self.device)
        if len(self._part_streams) < parts - 1:
            self._part_streams = lane_streams(self.device, max(3, parts - 1))[:parts - 1]  # (programs that split use no lanes: the lane streams serve)
            self._part_events = [torch.cuda.Event() for _ in range(parts)]
        e_fork = self._part_events[0]
        e_fork.record(cur)  # (the inputs are ready on the caller's stream, and what it ran before has read the buffers the parts write)
        self._phase_mark(cur, 0)
        res = [None] * parts
        for i in side:
            st = self._part_streams[i - 1]
            for t in inputs:
                t.record_stream(st)
            with torch.cuda.stream(st):
                st.wait_event(e_fork)
                res[i] = run_part(i)
                self._part_events[i].record(st)
        res[0] = run_part(0)
        for i in range(1, parts):
            cur.wait_event(self._part_events[i])
        self._phase_mark(cur, 1)
        return res

    # bench.py: the span of the CONCURRENT part-batch programs of a forward (fork -> join) between two timing events on the caller's
    # stream -- two markers per forward instead of one per launch, so the forward runs at its product speed (phase_events = [e0, e1]
    # armed by the caller; None = off)
    phase_events = None

    def _phase_mark(self, cur, which):
        if self.phase_events is not None:
            self.phase_events[which].record(cur)

    def program_bytes(self):
        """arena + workspace bytes held by the cached programs (bench.py --ragged-stream reports it)"""
        return sum(v[0].nbytes for v in self.programs.values())

    def _program(self, key, build):
        """LRU cache of programs, most recently used last; bounded by entries and by bytes (the newest program always stays)"""
        if key in self.programs:
            self.programs[key] = self.programs.pop(key)
        else:
            self.programs[key] = build()
            self.n_builds += 1
            while len(self.programs) > 1 and (len(self.programs) > self.MAX_PROGRAMS or self.program_bytes() > self.MAX_PROGRAM_BYTES):
                self.programs.pop(next(iter(self.programs)))
        return self.programs[key]

    def _run_towers(self, x, crop_bounds, H, W, flip, dest, dest_cap):
        """The per-crop tower (+ reduce) on the crops [crop_bounds[i], crop_bounds[i + 1]) of x as part program i, every part but the first on
        a stream of its own (_fork_parts; a single part runs on the caller's), each handing its features over with a row copy into
        rows of dest [dest_cap (x 2 with the flip test), h, w, cs]: the plain rows at the crops' own indices, the mirrored ones dest_cap
        behind them.  -> the part programs"""
        def run_tower(i):
            lo, hi = crop_bounds[i], crop_bounds[i + 1]
            capp = self.capacity(hi - lo)
            Pw, pw, f = self._program((capp, H, W, flip, "tower", i), lambda: self._build(capp, H, W, [1] * capp, flip, part="tower"))
            xi = x[lo:hi]
            pw["x"].in_ = xi.data_ptr()
            pw["x"].n_valid = hi - lo
            Pw.run()
            fv = f.view()
            dest[lo:hi].copy_(fv[:hi - lo])
            if flip:
                dest[dest_cap + lo:dest_cap + hi].copy_(fv[capp:capp + hi - lo])
            return Pw
        parts = len(crop_bounds) - 1
        return self._fork_parts(range(parts - 1, 0, -1), [x], run_tower) if parts > 1 else [run_tower(0)]

    def _forward_split(self, x, pos_mask, length, flip_joint_map, S, H, W, sine_n, bounds):
        """Models whose first stage is the bare HRNet tower (vanilla I2R-Net): the per-crop TOWER of every image group runs as its own
        program on its own stream, the rest of the forward -- position branch, inter-human encoder over ALL images (one launch per
        layer: 384 query tiles with the partial key split instead of two launches of 192), deconvs, head -- as one tail program on
        the caller's stream behind the join.  The towers hand their features over with a row copy into the tail's buffer."""
        flip = flip_joint_map is not None
        x = x.to(self.device).contiguous()
        cap = self.capacity(S)
        Pt, patch = self._program((cap, H, W, flip, "tail"), lambda: self._build(cap, H, W, list(length) + [1] * (cap - S), flip, part="tail"))
        progs = self._run_towers(x, [sum(length[:b]) for b in bounds], H, W, flip, patch["feat"].view(), cap)
        self.last_programs = progs + [Pt]
        self.last_concurrent = progs  # (ran side by side on their own streams: bench.py times them that way)
        return self._run_program(Pt, patch, None, pos_mask, length, flip_joint_map, S, cap, H, W, sine_n)

    # ---- grouped forward: person groups that share crops (the reference's PATCH_MODE main_target, input.main_target_groups) ----
    # The reference pushes every member of every group through the whole network.  The first stage is per crop, so here it runs once
    # per DISTINCT crop; only the part behind it sees the expanded batch, and only the first member of every group reaches the
    # up-sampling layers and the head.  Which crops make up which group is DATA of a call (two device tables), never part of a program.
    def _groups_shared(self, H, W, share=None):
        """How forward_groups runs: "tower" -- the first stage is the bare HRNet tower and the tower / tail seam serves the groups;
        "first" -- a first stage of its own (TransPose-H, HRFormer) once per crop, its tail on the gathered rows (share=True only);
        None -- the expanded forward.  share: forward_groups' share_first_stage.  ValueError: the stand-alone models, and a model whose
        tail cannot take gathered rows where the first stage would be shared (always for the bare tower unless share is False)."""
        if self.name not in ("interformer_pureMulti", "interformer", "interformer_2stage"):
            raise ValueError("forward_groups serves the inter-human models (MODEL.NAME %r has no person groups)" % self.name)
        if share is False:
            return None
        bare = (self.name == "interformer_pureMulti" or not self.singleformer) and isinstance(self.tower, HRNetW48)
        if not bare and share is None:
            return None
        if self.use_pos and self.pe_mode == "sine":
            raise ValueError("forward_groups: MULTI_POS_EMBEDDING sine is not served (its table depends on a crop's position inside the group)")
        if self.cat_concat:
            raise ValueError("forward_groups: MULTI_POS_EMBEDDING cat_vec concatenated is not served (the hand-over buffer is DIM_MODEL wide)")
        if self.window_attn:
            raise ValueError("forward_groups: ATTENTION_TYPE window is not served (its block re-views the whole batch's output)")
        if bare:
            return None if H % self.tower.stride or W % self.tower.stride else "tower"  # (the tower's and the tail's map sizes must agree, as in _split_bounds)
        tok = (H // 2 ** self.res_layer // 4) * (W // 2 ** self.res_layer // 4) if self.singleformer == "transpose_h" else None
        if H % 32 or W % 32 or (tok is not None and tok != self.single_tokens):
            raise ValueError("forward_groups: share_first_stage does not serve %d x %d inputs (the first stage is built for MODEL.IMAGE_SIZE; "
                             "maps of 1/32 of the input must exist)" % (H, W))
        return "first"

    @staticmethod
    def _first_rows(group_len):
        """row of every group's first member in the expanded batch"""
        out, r = [], 0
        for n in group_len:
            out.append(r)
            r += n
        return out

    def forward_groups(self, x, pos_mask, members, group_len, flip_joint_map=None, share_first_stage=None, persons=None, rollout=None, relations=None,
                       capture=None):
        """x [S, 3, H, W], pos_mask [S, 1, H, W]: the DISTINCT crops of a batch; members: device int32 [sum(group_len)] of crop indices in
        [0, S), group after group (input.main_target_groups); group_len: host list of the groups' sizes.  -> the 'multi' heat maps of the
        FIRST member of every group, [len(group_len), J, H/4, W/4] -- what the reference's validate_main_target keeps of model(x[members],
        pos_mask[members], group_len) (get_target_person, lib/core/function.py:309-334); with flip_joint_map merged with the flip test's.
        share_first_stage: None (default) -- models whose first stage is the bare HRNet tower run it once per crop (S, not
        sum(group_len), times) and the tail on the gathered rows, every other model runs the expanded forward; True -- the models with
        a first stage of their own (TransPose-H, HRFormer) share it too: first stage, pooling and position branch once per crop, ONE
        i2r_rows_gather_multi into group layout, the inter-human encoder, one more for the groups' first rows, the tail per group
        (ValueError where the tail cannot take gathered rows: sine, cat_vec concatenated, window, an unserved size); False -- always the
        expanded forward.  Programs are keyed by capacities only: other groups of the same sizes build nothing.  On every shared path
        (the default one of the HRNet tower included) a member index outside [0, S) is never dereferenced: the hand-over gathers are
        bound to the S real crops of the call, so its rows -- features, mask -- are zeros, never what a capacity slot holds.
        persons, rollout: ValueError when given -- the grouped forward has no attention-map capture (forward(..., capture=, persons=) has)
        but the target form:
        relations (attn_capture.TargetMaps, with capture = a set of (stack, layer) of the inter-human stack): the relations of every
        group's TARGET (its first member, the one whose heat maps are kept) to the group's members, of every captured layer, on whichever
        of the three ways the call runs -> (heat maps, (relation, maps)): relation[(stack, layer)] = per group a [m_g] view (sums to 1),
        maps[(stack, layer)] = per group a [m_g, h r, w r] view (relations.maps "dependency": where on member j the target looks,
        "affect": which of the target's tokens look at member j; None: no entry); views of one zeroed buffer in which group g's blocks
        start g * slots entries into their layer's set (include/i2r_hip.h: i2r_attn_target_maps).  One program per (capacities, capture
        set, mode, scale); other groups at the same capacities build nothing, and the default grouped programs are not touched.
        ValueError: the flip test, another stack's layer, the window-type block, persons= or rollout= too."""
        if persons is not None:
            raise ValueError("forward_groups: persons= is not served (no attention-map capture on the grouped forward)")
        if rollout is not None:
            raise ValueError("forward_groups: rollout= is not served (no attention-map capture on the grouped forward)")
        form = None
        if relations is not None:
            form = attn_capture.resolve(capture, None, None, flip_joint_map, self.capture_stacks(), self.inter_stack, self.window_attn, targets=relations)
        elif capture:
            raise ValueError("forward_groups: capture= goes with relations= (the target form is the grouped forward's only capture)")
        assert x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32
        assert share_first_stage in (None, True, False)
        S, _, H, W = x.shape
        group_len = [int(n) for n in group_len]
        assert group_len and all(n >= 1 for n in group_len), "every group needs at least one member"
        assert torch.is_tensor(members) and members.numel() == sum(group_len), "members: %d entries for groups of %d" % (members.numel(), sum(group_len))
        members = members.to(self.device, torch.int32).contiguous().view(-1)
        with torch.cuda.device(self.device):
            x = x.to(self.device).contiguous()
            pm = pos_mask.to(self.device, torch.float32).contiguous() if pos_mask is not None else None
            mode = self._groups_shared(H, W, share_first_stage)
            if mode is not None:
                return self._forward_groups_shared(mode, x, pm, members, group_len, flip_joint_map, S, H, W, form)
            # not shared: the reference's own arithmetic on the gathered inputs (index plumbing in torch, every launch in forward())
            idx = members.long()
            first = torch.tensor(self._first_rows(group_len), dtype=torch.long).to(self.device)
            if form:  # (one capture program over the expanded batch, as forward(..., capture=) runs its forms)
                y, res = self._forward_part(x.index_select(0, idx), pm.index_select(0, idx) if pm is not None else None, group_len, None, sum(group_len),
                                            H, W, max(group_len), form=form)
                return _multi(y).index_select(0, first), res
            y = _multi(self.forward(x.index_select(0, idx), pm.index_select(0, idx) if pm is not None else None, group_len, flip_joint_map))
            return y.index_select(0, first)

    def _build_groups(self, mode, capS, capG, capN, H, W, flip, form=None):
        """The program of a grouped forward behind the first stage: person-level features and position rows [capS] -> ONE rows_gather_multi
        (patch["hand_over"]) into group layout [capG] by the member table -> inter-human encoder -> one rows_gather_multi of the first row
        of every group [capN] -> _emit_tail.  With the flip test every buffer holds the mirrored half behind the plain one.
        mode "tower": the person features are a buffer that tower programs fill (patch["pfeat"], _run_towers); the members' MASKS are
        gathered (a segment whose source is the call's pos_mask) and the position branch runs on them.
        mode "first": the program holds the first stage too (no `single` head), pooling to TRANS_SIZE and the position branch on the
        distinct crops, bound straight to the call's pos_mask; its rows are gathered like the features, and for the tail the
        full-resolution first-stage features of every group's FIRST member [capN] by patch["first_member"].
        form: the target form (attn_capture.TargetForm) -- the inter-human encoder captures form.capture too (Program.bind_capture)."""
        P = self._new_program(form)
        patch, k, tw = {}, (2 if flip else 1), self.cfg["MODEL"]["TRANS_SIZE"][-1]
        g = pos = posg = sf = None
        if mode == "tower":
            f = patch["pfeat"] = P.alloc(k * capS, H // self.tower.stride, W // self.tower.stride, self.reduce.cout)
            f.t.zero_()
        else:
            g, patch["x"] = self._emit_single(P, k * capS, H, W, capS)
            f = self._pool_to_trans(P, g)
            if self.use_pos:
                pos, patch["pos_mask"] = self._pos_branch(P, k * capS, H, W, tw, n_src=capS)
                assert (pos.h, pos.w, pos.cs) == (f.h, f.w, f.cs)
        # the member table carries one more entry, always -1: where the capacity slots of the first-row table point (_forward_groups_shared)
        mtab = patch["members"] = torch.full((capG + 1,), -1, dtype=torch.int32, device=self.device)
        ftab = patch["first"] = torch.full((capN,), -1, dtype=torch.int32, device=self.device)
        fg = P.alloc(k * capG, f.h, f.w, f.c, f.dt)
        pairs = [(f, fg, mtab, capG)]
        if pos is not None:
            posg = P.alloc(k * capG, pos.h, pos.w, pos.c, pos.dt)
            pairs.append((pos, posg, mtab, capG))
        if mode == "first":
            fmtab = patch["first_member"] = torch.full((capN,), -1, dtype=torch.int32, device=self.device)  # members[first row of group]
            if self.domain_trans is not None or self.upconv is not None or self.deconvs:  # (the tail reads the first-stage features)
                sf = P.alloc(k * capN, g.h, g.w, g.c, g.dt)
                pairs.append((g, sf, fmtab, capN))
        segs = [(src, out, tab, n, capS, half * capS, half * n) for half in range(k) for src, out, tab, n in pairs]
        if mode == "tower" and self.use_pos:
            assert (H * W) % 4 == 0
            # the members' masks [capG, 1, H, W] (not mirrored: the stem kernel does that), outside the arena, whose rows are 16 channels wide
            gm = Act(torch.zeros(capG * H * W, dtype=torch.float32, device=self.device), capG, H, W, 1, 1)
            P.keep.append(gm.t)
            P.nbytes += gm.t.numel() * 4
            segs.append((_RawAct(0, gm, n=capS), gm, mtab, capG, capS, 0, 0))
        # (per call: n_src of every segment = the S real crops, src of the mask segment = the call's pos_mask)
        patch["hand_over"] = P.rows_gather_multi(segs)
        if mode == "first":
            P.release(g, f if f is not g else None, pos)
        if mode == "tower" and self.use_pos:
            patch["mask_seg"] = patch["hand_over"].seg[len(segs) - 1]
            posg, pe = self._pos_branch(P, k * capG, H, W, tw, n_src=capG)
            pe.in_, pe.n_valid = gm.ptr, capG
            assert (posg.h, posg.w, posg.cs) == (fg.h, fg.w, fg.cs)
        e = P.encoder(fg, self.layers, self._token_offsets([1] * (k * capG), fg.h * fg.w), pos=posg.ptr if posg is not None else 0,
                      regroupable=True, pre_norm=self.pre_norm, capture=self._capture_spec(form.capture, self.inter_stack, self.layers, d=fg.c) if form else None)
        e1 = P.alloc(k * capN, e.h, e.w, e.c, e.dt)
        P.rows_gather_multi([(e, e1, ftab, capN, capG, half * capG, half * capN) for half in range(k)])
        P.release(e)
        return self._emit_tail(P, patch, e1, sf)

    def _forward_groups_shared(self, mode, x, pm, members, group_len, flip_joint_map, S, H, W, form=None):
        flip = flip_joint_map is not None
        G, N = sum(group_len), len(group_len)
        capS, capG, capN = self.capacity(S), self.capacity(G), self.capacity(N)
        key = (capG, capN, capS, H, W, flip, "groups", mode)
        Pt, patch = self._program(key + form.key if form else key, lambda: self._build_groups(mode, capS, capG, capN, H, W, flip, form))
        progs = []
        if mode == "tower":  # (the tower is per crop: any cut of the S crops serves)
            progs = self._run_towers(x, self._split_bounds([1] * S, H, W) or [0, S], H, W, flip, patch["pfeat"].view(), capS)
        self.last_programs = progs + [Pt]
        self.last_concurrent = progs if len(progs) > 1 else []
        # bind the call: the crops, the masks, the tables, the token groups (capacity slots: one-person groups of zero rows)
        if self.use_pos:
            assert pm is not None and pm.shape == (S, 1, H, W)
        self._bind_inputs(patch, None if mode == "tower" else x, pm, S)
        for seg in patch["hand_over"].seg:
            seg.n_src = S  # (a member index beyond the real crops gives a zero row, not a capacity slot's)
        if "mask_seg" in patch:
            patch["mask_seg"].src = pm.data_ptr()
        patch["members"].fill_(-1)
        patch["members"][:G].copy_(members)
        fkey = tuple(group_len)
        if patch.get("_first_key") != fkey:
            first = self._first_rows(group_len)
            patch["first"].copy_(torch.tensor(first + [-1] * (capN - N), dtype=torch.int32).pin_memory(), non_blocking=True)
            if "first_member" in patch:
                patch["_first_idx"] = torch.tensor(first + [capG] * (capN - N), dtype=torch.long).to(self.device)
            patch["_first_key"] = fkey
        if "first_member" in patch:
            torch.index_select(patch["members"], 0, patch["_first_idx"], out=patch["first_member"])  # (on the device: nothing is read back)
        self._bind_groups(Pt, group_len, capG - G, flip)
        # (a capture: the call's real groups -- the capacity slots behind them are never among the computed groups)
        views = self._bind_capture(Pt, form, S, group_len, H, W) if form else None
        out = self._run_bound(Pt, patch, capN, N, flip_joint_map, H, W)[0]
        return (out, self._finish_capture(Pt, views, S, H)) if form else out

    def _forward_part(self, x, pos_mask, length, flip_joint_map, S, H, W, sine_n, slot=0, form=None):
        x = x.to(self.device).contiguous()
        flip = flip_joint_map is not None
        # one program per (capacity, H, W, flip): the launch list and every buffer depend on the crop capacity only; the
        # persons-per-image grouping enters through the encoder's offset table, the real crop count through the stem kernels
        cap = self.capacity(S)
        key = (cap, H, W, flip) if slot == 0 else (cap, H, W, flip, slot)  # (a Program owns its arena: the concurrent half needs its own)
        if self.window_attn:  # the padded person layout IS the program: no capacity slots, one program per `length`
            cap, key = S, (S, H, W, flip, "window", tuple(length))
        if form:
            key = key + form.key
        P, patch = self._program(key, lambda: self._build(cap, H, W, list(length) + [1] * (cap - S), flip, form=form))
        self.last_concurrent = []
        self.last_programs = [P]  # (_forward merges the parts')
        return self._run_program(P, patch, x, pos_mask, length, flip_joint_map, S, cap, H, W, sine_n, form)

    def _run_program(self, P, patch, x, pos_mask, length, flip_joint_map, S, cap, H, W, sine_n, form=None):
        """Bind one call into a built program of capacity `cap` and run it on the current stream: the token groups of `length` (capacity
        slots as one-person groups), the sine rows, the inputs (x None: tower programs filled patch["feat"]), fresh outputs, the capture
        buffers; then the flip merge and the slice to the S real crops.  -> what forward() returns."""
        glen = self._bind_groups(P, length, cap - S, flip_joint_map is not None)
        self._fill_sine(patch, glen, sine_n)
        pm = None
        if "pos_mask" in patch:
            pm = pos_mask.to(self.device, torch.float32).contiguous()
            assert pm.shape == (S, 1, H, W)
            if self.window_attn:  # one more crop: the zero mask of the padded persons (_emit_window_block)
                pm = torch.cat([pm, pm.new_zeros(1, 1, H, W)], 0)
        self._bind_inputs(patch, x, pm, S)
        views = self._bind_capture(P, form, S, length, H, W) if form else None
        multi, single = self._run_bound(P, patch, cap, S, flip_joint_map, H, W)
        res = {"single": single, "multi": multi} if single is not None else multi
        return (res, self._finish_capture(P, views, S, H, multi)) if form else res

    def _finish_capture(self, P, views, S, H, multi=None):
        """behind a capture program that has run: the work its form keeps behind the head (attn_bind: the joint form goes head ->
        i2r_joint_tokens on `multi` -> query launches), on the current stream, then what the caller gets of the bound `views`"""
        behind = attn_bind.PAIRS[P.form.behind][1](P, multi, S, H) if P.form.behind else None
        return P.form.result(views, lambda: self._capture_inputs(P, S), behind)

    # the per-call steps every bound forward shares (_run_program, _forward_groups_shared)
    def _bind_groups(self, P, length, pad, flip):
        """the token groups of a call: `length` persons per group, then `pad` capacity slots as one-person groups, all of it twice with the
        flip test -> that list"""
        glen = list(length) + [1] * pad
        if flip:
            glen = glen + glen
        for grouping, tok in P.groupings:
            P.set_groups(grouping, self._token_offsets(glen, tok))
        return glen

    @staticmethod
    def _bind_inputs(patch, x, pm, S):
        """the S crops x (None: tower programs read them) and the masks pm of a call, device tensors the caller holds until the run is
        issued, into the stem args of the program that reads them"""
        if x is not None:
            patch["x"].in_ = x.data_ptr()
            patch["x"].n_valid = S
        if "pos_mask" in patch:
            patch["pos_mask"].in_ = pm.data_ptr()
            patch["pos_mask"].n_valid = pm.shape[0]

    def _run_bound(self, P, patch, cap, S, flip_joint_map, H, W):
        """fresh outputs for the heads of a bound program of `cap` output rows, the run on the current stream, then the flip merge or the
        slice to the S real rows -> ('multi' maps, 'single' maps or None: a program without that head, the flip test)"""
        flip = flip_joint_map is not None
        out = torch.empty(2 * cap if flip else cap, self.cfg["MODEL"]["NUM_JOINTS"], H // 4, W // 4, dtype=torch.float32, device=self.device)
        patch["multi"].out = out.data_ptr()
        single = None
        if "single" in patch:
            single = torch.empty_like(out)
            patch["single"].out = single.data_ptr()
        P.run(self.side_streams if P.uses_lanes else None)
        if flip:
            return self._flip_merge(out, out[cap:], flip_joint_map, S, H, W), None
        return out[:S], (single[:S] if single is not None else None)
