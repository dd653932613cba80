"""GPU measurement aid: net.attention_at_joints (one forward, tables made on the device) against the two-call flow it replaces --
forward, arg-max on the device, .cpu(), attention_at (a second forward) -- at config 1's shape: vanilla I2R-Net (w48), 32 crops grouped
as bench.py groups them, all 6 layers of global_encoder, maps at input resolution, both modes.  Per mode: a warm-up of both flows, then
rounds that alternate the two flows in both orders (A B, B A, ...); every sample is a host clock around calls that end in a device
synchronise (the two-call flow synchronises in its middle by itself: that is what it costs).  Reported: the medians and the spread
(min, max) in us per call, and the bytes of fp32 q|k the joint program holds for its captured layers.
  python tools/time_attn_joints.py [--rounds N] [--calls N] [--json PATH]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import i2r_amd  # noqa: E402,F401
from i2r_amd import config, models, synth  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _sample(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    rounds, calls = _arg("--rounds", 6), _arg("--calls", 10)
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    cfg = config.load_config("w48_pure_en6")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False).cuda()
    x, m, length = synth.make_inputs([4] * 8, 256, 192)  # (the grouping bench.py gives this model)
    x, m = x.cuda(), m.cuda()
    S, J = sum(length), cfg.MODEL.NUM_JOINTS

    def two_calls(mode):
        y = net(x, m, length)
        flat = y.reshape(S, J, -1)
        top, idx = flat.amax(-1), flat.argmax(-1)
        idx = torch.where(top > 0, idx, torch.zeros_like(idx))
        pts = (4 * torch.stack([idx % y.shape[3], idx // y.shape[3]], -1)).cpu()
        return net.attention_at(x, m, length, pts, mode=mode)

    results = []
    for mode in ("dependency", "affect"):
        flows = {"joints_us": lambda: net.attention_at_joints(x, m, length, mode=mode), "two_call_us": lambda: two_calls(mode)}
        for fn in flows.values():  # warm-up: programs built, code objects loaded
            _sample(fn, 3)
        out, joints, _, maps = net.attention_at_joints(x, m, length, mode=mode)
        _, ref = two_calls(mode)
        same = all(torch.equal(u, v) for k in maps for u, v in zip(maps[k], ref[k]))
        samples = {k: [] for k in flows}
        for r in range(rounds):
            for k in (sorted(flows) if r % 2 == 0 else sorted(flows, reverse=True)):
                samples[k].append(_sample(flows[k], calls))
        eng = net.engine()
        prog = next(v[0] for k, v in eng.programs.items() if "joints" in k and k[k.index("query") + 1] == ("dependency", "affect").index(mode))
        held = sum(c.x.n * c.x.h * c.x.w * 4 * next(q.qk_cs for _, q in c.ops) * len(c.ops) for c in prog.captures)
        row = dict(config="1", model="w48_pure_en6", crops=S, length=length, mode=mode, layers=cfg.MODEL.ENCODER_LAYERS, rounds=rounds, calls_per_sample=calls,
                   maps_equal=bool(same), held_qk_bytes=int(held))
        for k, v in samples.items():
            row[k] = dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
        row["ratio_two_call_over_joints"] = round(row["two_call_us"]["median"] / row["joints_us"]["median"], 3)
        results.append(row)
        print(json.dumps(row))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
