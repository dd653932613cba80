"""GPU measurement aid: the attention maps at query points (i2r_attn_query_maps, Engine.forward(..., capture=, queries=)) of the two sizes
DESIGN.md quotes, beside the full capture tools/time_attn_maps.py times.  Meant to run under
    rocprofv3 --kernel-trace --stats -- python tools/time_attn_query.py [1|3 ...] [--json out.json]
(the stats CSV gives aq_row_stats_k / aq_rows_k / aw_stats_k / aq_cols_k / aq_upsample_k per launch); it prints per config and variant
(K = 19 points per crop, both modes, scale 1 and down_rate) the work one capture forward asks for, the bytes allocated for maps and
workspaces, and the host-timed difference between the capture forward and the default forward.
  config 1: vanilla I2R-Net, 8 images x 4 persons, the 6 layers of global_encoder (L = 768 per image, 76 queries per image)
  config 3: TransPose-H stand-alone, 57 crops, the 4 layers of global_encoder (L = 3072 per crop, 19 queries per crop)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import i2r_amd  # noqa: E402,F401
from i2r_amd import arch, config, models, synth  # noqa: E402
from i2r_amd.engine import AttnQueries  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.3e12  # fp32 matrix pipe, HBM (MI355X)
K_POINTS = 19  # 17 key points + two random ones (visualize.py)


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3  # us


def main():
    argv = sys.argv[1:]
    out_path = argv[argv.index("--json") + 1] if "--json" in argv else None
    which = [a for a in argv if a in ("1", "3")] or ["1", "3"]
    results = []
    for c in which:
        if c == "1":
            cfg = config.load_config("w48_pure_en6")
            net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False).cuda()
            length = [4] * 8
            x, m, length = synth.make_inputs(length, 256, 192)
            x, m = x.cuda(), m.cuda()
            eng = net.engine()
            fwd = lambda **kw: eng.forward(x, m, length, **kw)  # noqa: E731
            persons, n_iter = 4, 20
        else:
            cfg = config.load_config("tph_192_p6_b4")
            net = models.transpose_h.get_pose_net(cfg, is_train=False)
            net.load_state_dict(synth.make_state_dict(arch.transpose_h_spec(cfg, "")))
            net = net.cuda()
            x, _, _ = synth.make_inputs([1] * 57, 256, 192)
            x = x.cuda()
            eng = net.engine()
            fwd = lambda **kw: eng.forward_single(x, **kw)  # noqa: E731
            persons, n_iter = 1, 10
        stack, n_layers, heads, hp = "global_encoder", cfg.MODEL.ENCODER_LAYERS, cfg.MODEL.N_HEAD, 96
        fh, fw = eng.capture_map_sizes(256, 192)[stack]
        down = 256 // fh
        L, groups = persons * fh * fw, x.shape[0] // persons
        kq = persons * K_POINTS  # queries per group
        cap = {(stack, i) for i in range(n_layers)}
        tok = torch.from_numpy(np.random.RandomState(0).randint(0, L, size=(groups, kq)).astype(np.int32))
        t_def = _time(lambda: fwd(), n_iter)
        for mode in (0, 1):
            for scale in (1, down):
                q = AttnQueries({stack: tok}, mode, scale, capacity=K_POINTS)
                t_cap = _time(lambda: fwd(capture=cap, queries=q), n_iter)
                # executed Q K^T flops: mode 0 statistics + rows over the kq gathered queries; mode 1 the full statistics pass + kq columns
                qkt = 2 * heads * hp * (2 * kq * L if mode == 0 else L * L + kq * L)
                flop = n_layers * groups * qkt
                map_bytes = n_layers * groups * 4 * kq * L * scale * scale
                ws_bytes = 4 * (2 * heads * -(-L // 128) * (groups * kq if mode == 0 else groups * L) + (kq * groups * L if scale > 1 else 0))
                bound_us = max(flop / PEAK_FLOPS, map_bytes / PEAK_BYTES) * 1e6
                results.append(dict(config=c, mode=("dependency", "affect")[mode], scale=scale, layers=n_layers, tokens_per_entry=L, entries=groups,
                                    queries_per_entry=kq, executed_gflop=round(flop / 1e9, 3), map_mbytes=round(map_bytes / 1e6, 3),
                                    workspace_mbytes=round(ws_bytes / 1e6, 3), full_map_mbytes=round(n_layers * groups * 4 * L * L / 1e6, 1),
                                    roofline_us=round(bound_us, 2), forward_us=round(t_def, 1), capture_forward_us=round(t_cap, 1),
                                    capture_extra_us=round(t_cap - t_def, 1)))
                print(json.dumps(results[-1]))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
