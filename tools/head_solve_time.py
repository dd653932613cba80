"""GPU measurement aid for i2r_head_normal (the head re-fit's one-pass normal equations) beside i2r_head_grad from the same library:

    python tools/head_solve_time.py [--out profiles/head_solve_time.json] [--reps 30] [--fixture]
    rocprofv3 --kernel-trace --output-format csv -d D -- python tools/head_solve_time.py --reps 5     # a run of its own
    python tools/head_solve_time.py parse D profiles/head_solve_time.json

Per shape, device-event timed windows of REPS calls each, every window warmed up by one call of its own, the candidates taken in turn
ROUNDS times so that drift hits them alike:
  head_normal    caller.head_normal into one state, analytic form (tile launch + finish launch, workspace allocated per call)
  head_grad      caller.head_grad, analytic form
cold: every call reads another batch of a ring of feature batches larger than the 256 MB last-level cache; warm: one batch again and again.
solve_ms: HeadSolve.solve() on the accumulated state (the copy to the host, J eigendecompositions in numpy, the copy back), wall clock.
hbm_floor_us: the feature bytes of one batch read once at the HBM peak.  mfma_ideal_us: the v_mfma_f32_16x16x4_f32 instructions the tile
launch executes (Gram tiles ci <= cj and the blocks of r, four per 16-pixel fragment each; for i2r_head_grad both products), 32 cycles
each, spread evenly over 1024 SIMDs at 2.4 GHz.
--fixture: on the tph_l21 test fixture with the targets of tests/test_head_fit_gpu.py, how many HeadFit.step()s Adam at the cfg's rate
needs from the fresh initialisation to come within 1 % of the solved loss (capped at ADAM_CAP).
  config 1: 8 x 4 crops, 64 x 48, cin 96, 17 joints | config 3's batch: 57 crops, cin 96, 14 joints"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("config1_32crops_64x48_cin96_j17", 32, 17, 64, 48, 96), ("57crops_64x48_cin96_j14", 57, 14, 64, 48, 96)]
RING_BYTES = 512 << 20
ROUNDS = 3
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12
SIMDS, CLOCK_HZ, MFMA_CYCLES = 1024, 2.4e9, 32
ADAM_CAP = 20000


def mfma_counts(S, J, h, w, cin):
    """(head_normal, head_grad): matrix instructions of the tile launches"""
    frags, nf, cj = S * (-(-(h * w) // 16)), (1 if J <= 16 else 2), cin // 16
    return frags * 4 * (cj * (cj + 1) // 2 + nf * cj), frags * 4 * (2 * nf * cj)


def adam_steps_on_the_fixture(torch, caller):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _val_ref
    from _golden import setup
    from i2r_amd import models
    cfg, sd, x, m, length, g = setup("tph_l21")
    net = models.interformer.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    hi = net.head_input(x.cuda(), m.cuda(), length)
    S, h, w, _ = hi.feat.shape
    J = cfg.MODEL.NUM_JOINTS
    peak = _val_ref.max_preds(g["out_multi"]).astype(np.float64)
    offsets = np.array([[0.25, -0.25], [0.0, 0.3], [1.25, 0.0], [-0.3, 2.2], [4.25, 3.75], [-60.0, 0.25], [0.3, 80.0]])
    mu = peak + offsets[(np.arange(S)[:, None] * 3 + np.arange(J)[None, :]) % len(offsets)]
    vis = np.ones((S, J), np.float32)
    vis[0, 3] = vis[2, 5] = 0
    vis[1, 0] = 0.5
    kw = dict(joints_hm=torch.from_numpy(mu).cuda(), joints_vis=torch.from_numpy(vis).cuda())
    acc = caller.HeadSolve(hi.cin, J, cfg=cfg).add(hi.feat, **kw)
    solved = acc.head_fit()
    best = solved.grad(hi.feat, **kw).loss.item()
    torch.manual_seed(0)
    fit = caller.HeadFit(hi.cin, J, cfg=cfg)
    first = fit.grad(hi.feat, **kw).loss.item()
    steps, reached, losses = 0, None, []
    while steps < ADAM_CAP and reached is None:
        losses = [fit.step(hi.feat, **kw) for _ in range(200)]
        vals = torch.cat(losses).cpu().numpy()          # (the loss BEFORE each update)
        hit = np.nonzero(vals <= 1.01 * best)[0]
        if len(hit):
            reached = steps + int(hit[0])
        steps += 200
    return dict(fixture="tph_l21", crops=S, joints=J, cin=hi.cin, lr=cfg.TRAIN.LR, solved_loss=best, loss_at_the_fresh_head=first,
                adam_steps_to_within_1_percent=reached, cap=ADAM_CAP, loss_after_cap=None if reached is not None else float(vals[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fixture", action="store_true")
    args = ap.parse_args()
    import torch
    import i2r_amd  # noqa: F401
    from i2r_amd import caller
    if not torch.cuda.is_available():
        raise SystemExit("head_solve_time: no GPU -- a time is measured on the device or not at all")
    dev = torch.device("cuda", 0)
    out = {}
    for name, S, J, h, w, cin in SHAPES:
        rng = np.random.default_rng(1)
        mu = torch.from_numpy(np.stack([rng.uniform(-9, w + 9, (S, J)), rng.uniform(-9, h + 9, (S, J))], 2)).to(dev)
        vis = torch.from_numpy((rng.random((S, J)) > 0.2).astype(np.float32)).to(dev)
        feat_bytes = S * h * w * cin * 4
        n_ring = -(-RING_BYTES // feat_bytes)
        gen = torch.Generator(dev).manual_seed(2)
        ring = torch.randn(n_ring, S, h, w, cin, device=dev, generator=gen)
        wt = torch.randn(J, cin, 1, 1, device=dev, generator=gen) * 0.3 / cin ** 0.5
        b = torch.randn(J, device=dev, generator=gen) * 0.1
        acc = caller.HeadSolve(cin, J, device=dev)
        cands = (("head_normal", lambda i: acc.add(ring[i], joints_hm=mu, joints_vis=vis)),
                 ("head_grad", lambda i: caller.head_grad(ring[i], wt, b, joints_hm=mu, joints_vis=vis)))
        times = {(c, m): [] for c, _ in cands for m in ("cold", "warm")}
        for _ in range(ROUNDS):
            for mode in ("cold", "warm"):
                for cname, fn in cands:
                    fn(0)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for k in range(args.reps):
                        fn(k % n_ring if mode == "cold" else 0)
                    e1.record()
                    torch.cuda.synchronize()
                    times[(cname, mode)].append(e0.elapsed_time(e1) / args.reps * 1e3)
        solve_ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc.solve()
            torch.cuda.synchronize()
            solve_ms.append((time.perf_counter() - t0) * 1e3)
        nbytes = caller.ctypes.c_int64(0)
        caller.cabi.check(caller.cabi.lib().i2r_head_normal_ws_bytes(S, h, w, cin, J, caller.ctypes.byref(nbytes)))
        mn, mg = mfma_counts(S, J, h, w, cin)
        row = dict(crops=S, joints=J, h=h, w=w, cin=cin, feature_bytes=feat_bytes, workspace_bytes=nbytes.value, ring_batches=n_ring, reps=args.reps,
                   rounds=ROUNDS, calls_accumulated=int(acc.state.n.item()) // (S * h * w),
                   hbm_floor_us=dict(at_8_0_tb_s_spec=round(feat_bytes / HBM_PEAK * 1e6, 2), at_6_29_tb_s_copy=round(feat_bytes / HBM_COPY * 1e6, 2)),
                   mfma=dict(head_normal=mn, head_grad=mg, ratio=round(mn / mg, 3)),
                   mfma_ideal_us=dict(head_normal=round(mn * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e6, 2), head_grad=round(mg * MFMA_CYCLES / SIMDS / CLOCK_HZ * 1e6, 2)),
                   solve_ms=dict(median=round(float(np.median(solve_ms)), 2), min=round(min(solve_ms), 2), max=round(max(solve_ms), 2)))
        for (cname, mode), v in times.items():
            row["%s_%s_call_us" % (cname, mode)] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        del ring
    res = dict(what="time per call in microseconds between two device events around REPS calls (host launch cost included: it is what a fit loop "
                    "pays), median / min / max over ROUNDS windows; cold = features from HBM, warm = from the caches", shapes=out)
    if args.fixture:
        res["adam_against_the_closed_form"] = adam_steps_on_the_fixture(torch, caller)
        print(json.dumps(res["adam_against_the_closed_form"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def parse(d, into):
    """kernel times out of a rocprofv3 --kernel-trace run of its own (tracing slows the host: the call times come from a run without it),
    added to the JSON `into` under kernel_us.  The two shapes run different instantiations of the tile kernels (J 17: two joint fragments,
    J 14: one), which tells them apart by name; the finish launches are split by their order."""
    import csv
    import glob
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))

    def dur(r):
        return (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3

    def stat(v):
        return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2), launches=len(v)) if v else None
    res = json.load(open(into))
    for k, (name, S, J, h, w, cin) in enumerate(SHAPES):
        nf = 1 if J <= 16 else 2
        e = {}
        for kern in ("head_normal", "head_grad"):
            head = "%s_tile_k<%d, " % (kern, nf)
            e[kern + "_tile"] = stat([dur(r) for r in rows if head in r["Kernel_Name"]])
            fin = [dur(r) for r in rows if kern + "_finish_k" in r["Kernel_Name"]]
            e[kern + "_finish"] = stat(fin[k * len(fin) // len(SHAPES):(k + 1) * len(fin) // len(SHAPES)])
        res["shapes"][name]["kernel_us"] = e
    res["kernel_us"] = "rocprofv3 --kernel-trace, a run of its own: duration of every launch of the tile kernels (cold and warm windows together) and of the finish kernels"
    with open(into, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({n: v["kernel_us"] for n, v in res["shapes"].items()}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[3])
    else:
        main()
