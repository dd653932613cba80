"""GPU measurement aid: the target form of the attention per person (i2r_attn_target_maps, net.main_target_relations) beside the person
form (i2r_attn_person_maps) on the same grouped shape -- vanilla W48 at 256 x 192 (one head of 96, 192 tokens per person), 32 groups of
MAX_PATCH members.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_attn_target.py kernel M MODE
        one layer's launch of both forms, alternating (person, target, person, target, ...), N times each, in a profiler run of its own
    python tools/time_attn_target.py parse OUT.json M MODE STATS.csv [M MODE STATS.csv ...]
        kernel_stats CSVs of such runs -> per (M, MODE) the time per call of either form (the sum of its kernels' averages), their
        ratio, and beside it the ratio the work-item counts promise -- an expectation, not a result
    python tools/time_attn_target.py model OUT.json
        one main_target_relations call against forward_main_target + person_relations on the expanded batch (what gives the same
        numbers without the target form), device-event timed, 8 images x 4 persons, MAX_PATCH 3 and 6 (6: groups of 4)"""
import csv
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import i2r_amd  # noqa: E402,F401
from i2r_amd import cabi, config, models, synth  # noqa: E402
from i2r_amd import input as i2r_input  # noqa: E402

GROUPS, SEG, HEADS, HP, H, W, N = 32, 192, 1, 96, 16, 12, 20


def items(m, mode):
    """one-wave work items per call of (person form, target form) for GROUPS groups of m members, and the score tiles (16 queries x 16
    keys, per head) they compute -- the arithmetic of both forms is their score tiles"""
    L, q, kt = m * SEG, -(-SEG // 16), -(-SEG // 16)
    person = dict(stats=-(-L // 16) * -(-L // 128), affect=-(-L // 16) * m, depend=m * -(-L // 32) if mode == 1 else 0, relation=m * m)
    target = dict(stats=q * -(-L // 128), affect=q * m, depend=-(-L // 32) if mode == 1 else 0, relation=m)
    tiles = lambda it, rows: it["stats"] * 8 + it["affect"] * kt + it["depend"] * rows * 2  # (a 128-key block: 8 tiles; a 32-key block: 2 per query tile)
    return ({k: GROUPS * v for k, v in person.items()}, {k: GROUPS * v for k, v in target.items()}, tiles(person, q) * GROUPS, tiles(target, q) * GROUPS)


def kernel(m, mode):
    L = m * SEG
    n_tok = GROUPS * L
    g = torch.Generator(device="cuda").manual_seed(m)
    qk = torch.randn(n_tok, 2 * HP, device="cuda", generator=g) * HP ** -0.25
    offs = [i * L for i in range(GROUPS + 1)]
    goff = torch.tensor(offs, dtype=torch.int32, device="cuda")
    host_off = (ctypes.c_int32 * (GROUPS + 1))(*offs)
    stride = 2 * HEADS * -(-L // 128)
    ws = torch.empty(stride * n_tok, device="cuda")
    rows = torch.empty(2 * m * n_tok, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    calls = []
    for cls, fn, rel_n, map_n in ((cabi.AttnPersonArgs, cabi.lib().i2r_attn_person_maps, m * m, m * L), (cabi.AttnTargetArgs, cabi.lib().i2r_attn_target_maps, m, L)):
        rel, maps = torch.empty(GROUPS * rel_n, device="cuda"), torch.empty(GROUPS * map_n, device="cuda")
        r_off = torch.arange(GROUPS, dtype=torch.int64, device="cuda") * rel_n
        m_off = torch.arange(GROUPS, dtype=torch.int64, device="cuda") * map_n
        a = cls(qk=qk.data_ptr(), grp_off=goff.data_ptr(), ws=ws.data_ptr(), rel=rel.data_ptr(), rel_off=r_off.data_ptr(), maps=maps.data_ptr(),
                maps_off=m_off.data_ptr(), rows=rows.data_ptr(), grp_off_host=ctypes.cast(host_off, ctypes.c_void_p), n_grp=GROUPS, heads=HEADS, hp=HP,
                k_off=HP, qk_cs=2 * HP, ws_stride=stride, seg=SEG, mode=mode, scale=1, h=H, w=W)
        calls.append((fn, a, (rel, maps, r_off, m_off)))
    for _ in range(N + 2):  # (two warm-up rounds are in the averages of both forms alike)
        for fn, a, _keep in calls:
            cabi.check(fn(ctypes.byref(a), st), "launch")
    torch.cuda.synchronize()
    print(json.dumps(dict(m=m, mode=mode, calls=N + 2)))


def parse(out_path, triples):
    res = []
    for m, mode, path in triples:
        per = {"person": {}, "target": {}}
        with open(path) as f:
            for r in csv.DictReader(f):
                k = re.search(r"\b(aw_stats_k|a[pt]_(?:stats|affect|depend|relation)_k)\b", r["Name"])
                if k:
                    form = "target" if k.group(1).startswith("at_") else "person"
                    per[form][k.group(1)] = round(per[form].get(k.group(1), 0.0) + float(r["AverageNs"]) / 1e3, 2)
        pi, ti, pt, tt = items(m, mode)
        tp, tg = sum(per["person"].values()), sum(per["target"].values())
        res.append(dict(shape="vanilla W48 256x192, %d groups" % GROUPS, max_patch=m, mode=mode, person_us=round(tp, 1), target_us=round(tg, 1),
                        measured_ratio=round(tg / tp, 3) if tp else None, expected_ratio_score_tiles=round(tt / pt, 3), expected_about=round(1.0 / m, 3),
                        person_kernels_us=per["person"], target_kernels_us=per["target"], person_items=pi, target_items=ti))
        print(json.dumps(res[-1]))
    old = json.load(open(out_path)) if os.path.exists(out_path) else {}
    old["kernels"] = res
    json.dump(old, open(out_path, "w"), indent=1)


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def model(out_path):
    cfg = config.load_config("w48_pure_en6")
    net = models.interformer_pureMulti.get_pose_net(cfg, is_train=False).cuda()
    length = [4] * 8
    x, m, _ = synth.make_inputs(length, 256, 192)
    x, m = x.cuda(), m.cuda()
    boxes = (torch.rand(sum(length), 4, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 200).numpy()
    res = []
    for p in (3, 6):
        groups = i2r_input.main_target_groups(boxes, length, p, "cuda")
        idx = groups.members.long()
        xe, me = x[idx].contiguous(), m[idx].contiguous()
        for maps in (None, "dependency"):
            t_fwd = _time(lambda: net.forward_main_target(x, m, length, boxes, max_patch=p), N)
            t_new = _time(lambda: net.main_target_relations(x, m, length, boxes, max_patch=p, maps=maps), N)
            t_old = _time(lambda: (net.forward_main_target(x, m, length, boxes, max_patch=p), net.person_relations(xe, me, groups.group_len, maps=maps)), N)
            res.append(dict(max_patch=p, maps=maps, persons=sum(length), forward_main_target_us=round(t_fwd, 1), main_target_relations_us=round(t_new, 1),
                            forward_main_target_plus_person_relations_expanded_us=round(t_old, 1)))
            print(json.dumps(res[-1]))
    old = json.load(open(out_path)) if os.path.exists(out_path) else {}
    old["model"] = res
    json.dump(old, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel(int(sys.argv[2]), int(sys.argv[3]))
    elif sys.argv[1] == "parse":
        a = sys.argv[3:]
        parse(sys.argv[2], [(int(a[i]), int(a[i + 1]), a[i + 2]) for i in range(0, len(a), 3)])
    else:
        model(sys.argv[2])
