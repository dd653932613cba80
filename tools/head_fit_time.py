"""GPU measurement aid for i2r_head_grad (the head re-fit's fused gradient kernel):

    python tools/head_fit_time.py [--out profiles/head_fit_time.json] [--reps 30]

Per shape, device-event timed windows of REPS calls each, every window warmed up by one call of its own, the three candidates taken in
turn ROUNDS times so that drift hits them alike:
  head_grad      caller.head_grad, analytic form (i2r_head_grad: tile launch + finish launch, workspace allocated per call)
  head_grad_tensor  the same with the tensor-form target (the maps are read, not evaluated)
  torch          the composition it replaces, on the same device: caller.joint_targets -> NCHW copy of the features -> F.conv2d -> the loss of
                 JointsMSELoss -> autograd (torch_cl: the same without the copy, on a channels-last view)
cold: every call reads another batch of a ring of feature batches larger than the 256 MB last-level cache (the features come from HBM,
as they do behind a forward of another batch); warm: one batch again and again.
hbm_floor_us: the feature bytes of one batch read once at the HBM peak (8.0 TB/s spec; 6.29 TB/s is what a float4 copy measures).
Also printed: the largest |difference| of the gradients of the two paths relative to max |dw|, so that a time is never quoted for a
result that differs.
  config 1: 8 x 4 crops, 64 x 48, cin 96, 17 joints | config 3's batch: 57 crops, cin 96, 14 joints"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("config1_32crops_64x48_cin96_j17", 32, 17, 64, 48, 96), ("57crops_64x48_cin96_j14", 57, 14, 64, 48, 96)]
RING_BYTES = 512 << 20
ROUNDS = 3
HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import i2r_amd  # noqa: F401
    from i2r_amd import caller
    if not torch.cuda.is_available():
        raise SystemExit("head_fit_time: no GPU -- a time is measured on the device or not at all")
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
        wt = (torch.randn(J, cin, 1, 1, device=dev, generator=gen) * 0.3 / cin ** 0.5).requires_grad_()
        b = (torch.randn(J, device=dev, generator=gen) * 0.1).requires_grad_()
        target, tw = caller.joint_targets(mu, vis, (w, h))

        def fused(i):
            return caller.head_grad(ring[i], wt, b, joints_hm=mu, joints_vis=vis)

        def fused_tensor(i):
            return caller.head_grad(ring[i], wt, b, target, tw)

        def composed(i, copy=True):
            t, tws = caller.joint_targets(mu, vis, (w, h))
            x = ring[i].permute(0, 3, 1, 2)
            o = F.conv2d(x.contiguous() if copy else x, wt, b)
            tws = tws.view(S, J, 1, 1)
            loss = (0.5 * ((o * tws - t * tws) ** 2).mean((0, 2, 3))).sum() / J
            wt.grad = b.grad = None
            loss.backward()
            return loss

        cands = (("head_grad", fused), ("head_grad_tensor", fused_tensor), ("torch", composed), ("torch_cl", lambda i: composed(i, False)))
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
        g = fused(0)
        composed(0)
        rel = float((g.dw - wt.grad.view(J, cin)).abs().max() / wt.grad.abs().max())
        relb = float((g.db - b.grad).abs().max() / b.grad.abs().max())
        row = dict(crops=S, joints=J, h=h, w=w, cin=cin, feature_bytes=feat_bytes, ring_batches=n_ring, reps=args.reps, rounds=ROUNDS,
                   flop=4 * S * h * w * cin * J,
                   hbm_floor_us=dict(at_8_0_tb_s_spec=round(feat_bytes / HBM_PEAK * 1e6, 2), at_6_29_tb_s_copy=round(feat_bytes / HBM_COPY * 1e6, 2)),
                   dw_max_diff_rel_to_torch=rel, db_max_diff_rel_to_torch=relb)
        for (cname, mode), v in times.items():
            row["%s_%s_call_us" % (cname, mode)] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1), max=round(max(v), 1))
        for mode in ("cold", "warm"):
            row["torch_over_head_grad_%s" % mode] = round(row["torch_%s_call_us" % mode]["median"] / row["head_grad_%s_call_us" % mode]["median"], 2)
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        del ring
    res = dict(what="time per call in microseconds between two device events around REPS calls (host launch cost included: it is what a fit loop "
                    "pays), median / min / max over ROUNDS windows; cold = features from HBM, warm = from the caches", shapes=out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


def parse(d, into):
    """kernel times out of a `rocprofv3 --kernel-trace --output-format csv -d D -- python tools/head_fit_time.py` run of its own (tracing
    slows the host: the call times above come from a run without it), added to the JSON `into` under kernel_us.  The two shapes run
    different instantiations of the tile kernel (J 17: two joint fragments, J 14: one), which tells them apart by name."""
    import csv
    import glob
    (trace,) = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))

    def stat(v):
        return dict(median=round(float(np.median(v)), 2), min=round(min(v), 2), max=round(max(v), 2), launches=len(v))
    res = json.load(open(into))
    fin = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "head_grad_finish_k" in r["Kernel_Name"]]
    for k, (name, S, J, h, w, cin) in enumerate(SHAPES):
        nf = 1 if J <= 16 else 2
        e = {}
        for form, flag in (("analytic", "true"), ("tensor", "false")):
            head, tail = "head_grad_tile_k<%d, " % nf, ", %s>" % flag
            e["tile_" + form] = stat([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
                                      if head in r["Kernel_Name"] and tail in r["Kernel_Name"]])
        e["finish"] = stat(fin[k * len(fin) // len(SHAPES):(k + 1) * len(fin) // len(SHAPES)])
        res["shapes"][name]["kernel_us"] = e
    res["kernel_us"] = "rocprofv3 --kernel-trace, a run of its own: duration of every launch of the tile kernel (cold and warm windows together) and of the finish kernel"
    with open(into, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({n: v["kernel_us"] for n, v in res["shapes"].items()}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "parse":
        parse(sys.argv[2], sys.argv[3])
    else:
        main()
