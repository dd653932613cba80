"""GPU measurement aid: the attention-map capture launches (i2r_attn_weights) of the two sizes DESIGN.md quotes.  Meant to run under
    rocprofv3 --kernel-trace --stats -- python tools/time_attn_maps.py [1|3 ...]
(the stats CSV gives aw_stats_k / aw_probs_k per launch); it also prints per config the work one capture forward asks for and the
host-timed difference between the capture forward and the default forward.
  config 1: vanilla I2R-Net, 8 images x 4 persons, the 6 layers of global_encoder (L = 768 per image)
  config 3: TransPose-H stand-alone, 57 crops, the 4 layers of global_encoder (L = 3072 per crop, 8.6 GB of maps)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import i2r_amd  # noqa: E402,F401
from i2r_amd import arch, config, models, synth  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.3e12  # fp32 matrix pipe, HBM (MI355X)


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
    which = sys.argv[1:] or ["1", "3"]
    for c in which:
        if c == "1":
            cfg = config.load_config("w48_pure_en6")
            net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False).cuda()
            x, m, length = synth.make_inputs([4] * 8, 256, 192)
            x, m = x.cuda(), m.cuda()
            eng = net.engine()
            stack, n_layers, heads, hp = "global_encoder", cfg.MODEL.ENCODER_LAYERS, cfg.MODEL.N_HEAD, 96
            cap = {(stack, i) for i in range(n_layers)}
            default = lambda: eng.forward(x, m, length)  # noqa: E731
            capture = lambda: eng.forward(x, m, length, capture=cap)  # noqa: E731
            lens = [4 * 192] * 8
        else:
            cfg = config.load_config("tph_192_p6_b4")
            net = models.transpose_h.get_pose_net(cfg, is_train=False)
            net.load_state_dict(synth.make_state_dict(arch.transpose_h_spec(cfg, "")))
            net = net.cuda()
            x, _, _ = synth.make_inputs([1] * 57, 256, 192)
            x = x.cuda()
            eng = net.engine()
            stack, n_layers, heads, hp = "global_encoder", cfg.MODEL.ENCODER_LAYERS, cfg.MODEL.N_HEAD, 96
            cap = {(stack, i) for i in range(n_layers)}
            default = lambda: eng.forward_single(x)  # noqa: E731
            capture = lambda: eng.forward_single(x, capture=cap)  # noqa: E731
            lens = [3072] * 57
        n = 5 if c == "3" else 20
        t_def = _time(default, n)
        t_cap = _time(capture, n)
        qkt = n_layers * sum(2 * L * L * heads * hp for L in lens)  # one Q K^T per head (hp = the padded head dim the pipe executes)
        flop = 2 * qkt  # executed: the statistics pass and the probability pass both recompute Q K^T
        nbytes = n_layers * sum(4 * L * L for L in lens)
        bound_us = max(flop / PEAK_FLOPS, nbytes / PEAK_BYTES) * 1e6
        print(json.dumps(dict(config=c, layers=n_layers, tokens_per_entry=lens[0], entries=len(lens), qkt_gflop=round(qkt / 1e9, 2),
                              executed_gflop=round(flop / 1e9, 2), map_gbytes=round(nbytes / 1e9, 3), roofline_us=round(bound_us, 1),
                              forward_us=round(t_def, 1), capture_forward_us=round(t_cap, 1), capture_extra_us=round(t_cap - t_def, 1))))


if __name__ == "__main__":
    main()
