"""-m gpu: the path's one collective on hardware.  A 1-GPU box still runs RCCL: backend 'nccl' with world_size 1 exercises communicator
creation, all_gather_into_tensor on device buffers produced by a real forward, the async handle and the key-point payload (the driver's
8-GPU run is the only place a multi-rank RCCL ring exists; tests/test_dist.py covers world_size 2 on gloo)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist

from _golden import setup
from i2r_amd import caller, models
from i2r_amd import dist as i2r_dist

pytestmark = pytest.mark.gpu


@pytest.fixture()
def nccl_world1():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_rccl_gather_after_real_forward(nccl_world1):
    cfg, sd, x, m, length, g = setup("w48_l213")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    lo, hi, off = i2r_dist.shard_images(length, 0, 1)
    assert (lo, hi, off) == (0, len(length), 0)
    y = net(x.cuda(), m.cuda(), length)
    counts = [sum(length)]
    full = i2r_dist.gather_heatmaps(y, counts)
    assert full.is_cuda and torch.equal(full, y)
    h1 = i2r_dist.gather_heatmaps_async(y, counts)          # collective of step k in flight while step k+1 is issued (bench.py pattern)
    y2 = net(x.cuda(), m.cuda(), length)
    h2 = i2r_dist.gather_heatmaps_async(y2, counts)
    assert torch.equal(h1.wait(), y) and torch.equal(h2.wait(), y2) and torch.equal(y, y2)
    # the default payload: key points decoded on the device, [S, J, 3]
    preds, maxv = caller.decode(y, None, None, cfg.TEST.BLUR_KERNEL, transform_back=False)
    kp = i2r_dist.gather_keypoints(preds, maxv, counts)
    assert kp.shape == (sum(length), cfg.MODEL.NUM_JOINTS, 3)
    assert torch.equal(kp[..., :2], preds) and torch.equal(kp[..., 2:], maxv)
    kp2 = i2r_dist.gather_keypoints(preds, maxv, counts, async_op=True).wait()
    assert torch.equal(kp2, kp)
    t = torch.ones(1, device="cuda")
    dist.all_reduce(t)                                       # bench.py's max-over-ranks timing reduction
    assert t.item() == 1.0


def test_post_step_on_side_stream_equals_direct_gather(nccl_world1):
    """dist.PostStep (bench.py's data-parallel step): decode + asynchronous all-gather issued on a side stream under the NEXT forward --
    three consecutive steps give what the direct calls on the caller's stream give, in order, for both payloads."""
    cfg, sd, x, m, length, g = setup("w48_l213")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    counts = [sum(length)]
    dec = lambda t: caller.decode(t, None, None, cfg.TEST.BLUR_KERNEL, transform_back=False)
    kp_step = i2r_dist.PostStep(torch.device("cuda", 0), counts, decode=dec)
    hm_step = i2r_dist.PostStep(torch.device("cuda", 0), counts)
    xs = [x.cuda() * s for s in (1.0, 0.5, 0.25)]
    hs = []
    for xi in xs:  # (the handle of step k is only waited for by the side stream while step k + 1 is issued)
        y = net(xi, m.cuda(), length)
        hs.append((kp_step(y), hm_step(y)))
    last_kp, last_hm = kp_step.result(), hm_step.result()
    torch.cuda.synchronize()
    for i, xi in enumerate(xs):
        y = net(xi, m.cuda(), length)
        preds, maxv = dec(y)
        kp = torch.cat([preds, maxv], 2)
        got_kp, got_hm = (last_kp, last_hm) if i == len(xs) - 1 else (hs[i][0].out, hs[i][1].out)
        assert torch.equal(got_kp.view_as(kp), kp) and torch.equal(got_hm.view_as(y), y)


def _bench(*args, timeout=900, full=True):
    """bench.py as the driver runs it (a process of its own), -> its one JSON line.  full: --full without the roofline, CPU baseline and
    other workloads (parity and gather_alt stay); else the plain run"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT") and not k.startswith("I2R_")}
    opts = ["--full", "--no-cpu-baseline", "--no-roofline", "--no-other-workloads"] if full else []
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + opts + list(args),
                       cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    (line,) = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return json.loads(line)


def test_bench_strong_scaling_end_to_end_on_one_gpu():
    """`bench.py --gpus 1 --scaling strong --world1-collective`: the real model over the FIXED 64-image job (4 forwards of uneven crop
    counts per step), their rows gathered together through an RCCL process group of one rank -- every piece of the N > 1 strong-scaling
    step except the second GPU.  The line carries `shards`, the parity of image 0 holds, the value is positive."""
    out = _bench("--gpus", "1", "--scaling", "strong", "--steps", "3", "--warmup", "1", "--world1-collective")
    sh = out["shards"]
    assert out["scaling"] == "strong" and sh["images_total"] == 64 and sh["crops_per_rank"] == [sh["crops_total"]] and sh["forwards_per_rank_step"] == [4]
    assert "dp1" in out["config"]["parallelism"] and out["gather_alt"]["payload"] == "heatmaps"
    assert out["value"] > 1000 and out["parity"]["ok"]


def test_bench_config4_with_collective_matches_plain_line():
    """BASELINE configs[3] (HRFormer-B bf16, 16 crops per GPU -- the workload BASELINE quotes on 8 GPUs) at N = 1 with the per-step
    key-point all-gather and the max-over-ranks reduction in place (one-rank RCCL group) against the plain N = 1 line: both agree with
    the oracle and carry the same workload.  The throughput ratio of the two lines is a MEASUREMENT, not a correctness property: it is
    printed here and recorded by tools/collective_overhead.py -> profiles/round6_collective.json; it gates nothing."""
    plain = _bench("--config", "hrt_192_p4_b4", "--gpus", "1", "--steps", "10", "--warmup", "5")
    coll = _bench("--config", "hrt_192_p4_b4", "--gpus", "1", "--steps", "10", "--warmup", "5", "--world1-collective")
    assert plain["parity"]["ok"] and coll["parity"]["ok"]
    assert "dp1" in coll["config"]["parallelism"] and coll["config"]["crops_per_gpu_step"] == 16
    assert plain["value"] > 0 and coll["value"] > 0
    print("collective/plain throughput at N=1 (recorded, not asserted): %.1f / %.1f = %.3f" % (coll["value"], plain["value"], coll["value"] / plain["value"]))


def test_bench_plain_line_is_the_headline():
    """`bench.py --gpus 1 --steps K --warmup W` without --full: the headline of the timed steps and the lane map, none of the legs that
    --full runs after the timed region"""
    out = _bench("--gpus", "1", "--steps", "3", "--warmup", "2", full=False)
    assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 1000
    assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"] == "f32" and out["n_gpus"] == 1
    assert not out["lanes"]["device_side_waits_timed_out"]
    for k in ("roofline", "parity", "cpu_baseline", "other_workloads", "collective_overhead", "gather_alt"):
        assert k not in out, k
