"""GPU measurement aid: the attention per person (i2r_attn_person_maps, net.person_relations) at config 1's size, beside the full capture
tools/time_attn_maps.py and the query form tools/time_attn_query.py time the same way: per mode (None, dependency, affect; maps at
input resolution) the host-timed difference between the capture forward and the default forward.  host_issue_us is the time the
host alone spends per call (bind + launch, nothing waited for): the share that the capture's host side (attn_capture.py,
Program.bind_capture) can move.
  config 1: vanilla I2R-Net, 8 images x 4 persons, the 6 layers of global_encoder (L = 768 per image)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import i2r_amd  # noqa: E402,F401
from i2r_amd import config, models, synth  # noqa: E402


def _time(fn, n):
    """-> (us per call by device events, us per call the host spent issuing)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3, host / n * 1e6


def main():
    out_path = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    cfg = config.load_config("w48_pure_en6")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False).cuda()
    x, m, length = synth.make_inputs([4] * 8, 256, 192)
    x, m = x.cuda(), m.cuda()
    t_def, h_def = _time(lambda: net(x, m, length), 20)
    results = []
    for maps in (None, "dependency", "affect"):
        t_cap, h_cap = _time(lambda: net.person_relations(x, m, length, maps=maps, upsample=True), 20)
        results.append(dict(config="1", maps=maps, layers=cfg.MODEL.ENCODER_LAYERS, forward_us=round(t_def, 1), capture_forward_us=round(t_cap, 1),
                            capture_extra_us=round(t_cap - t_def, 1), host_issue_us=round(h_cap, 1), default_host_issue_us=round(h_def, 1)))
        print(json.dumps(results[-1]))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
