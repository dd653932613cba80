"""A/B of the 16-bit encoder kernels (enc_kv_lp_k, enc_layer_lp_k, enc_layer_lp4_k of csrc/i2r_encoder.hip) between two builds of the
library, one process per library (I2R_TOOL_LIB, as tools/enc_ab.py):
    I2R_TOOL_LIB=<lib> python tools/enc_lp_ab.py dump OUT.pt      the K and V buffers of i2r_encoder_kv and the output of i2r_encoder_layer for
                                                                   every case below (big: write OUT.pt to a temporary directory)
    python tools/enc_lp_ab.py compare A.pt B.pt OUT.json           torch.equal per buffer -> OUT.json; exit status 1 on any difference
    I2R_TOOL_LIB=<lib> python tools/enc_lp_ab.py time              the timing inputs, 20 launches each: run it under rocprofv3 --kernel-trace --stats
    python tools/enc_lp_ab.py times OUT.json P1.csv N1.csv P2.csv N2.csv   kernel_stats CSVs of the runs parent, new, parent, new -> OUT.json
Cases: the long-group cases of tests/test_kernels_gpu.py (both kernels: the engine's choice and n_qtiles192 = 0), the cases of
test_encoder_layer_low_precision, one config-3-shaped layer (57 crops x 768 tokens, d = 96, bf16, table pos) and one config-5-shaped layer
(one group of 12 x 432 tokens, d = 78, fp16).  Timing inputs: the last two, and the config-3 shape with n_qtiles192 = 0."""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch

KERNELS = ("enc_kv_lp_k", "enc_layer_lp_k", "enc_layer_lp4_k")


def _setup():
    import i2r_amd  # noqa: F401
    from i2r_amd import cabi
    if os.environ.get("I2R_TOOL_LIB"):
        cabi._LIB = cabi.load_library(os.path.join(ROOT, os.environ["I2R_TOOL_LIB"]))
    import test_kernels_gpu as T
    return T


def _layer(T, P, precision, d, sd, feat, offs, pos=None, table=None, one_wave=False):
    """one 16-bit layer on program P -> (descriptor, out Act); one_wave: n_qtiles192 = 0 (enc_layer_lp_k with QF = 4 on long-group inputs)"""
    from i2r_amd import engine
    dev = torch.device(T.DEV)
    L = engine.Packer(sd, dev, precision).encoder_layer("L", d, 192)
    if table is not None:
        tdev = table.to(dev)
        P.keep.append(tdev)
        out = P.encoder(T.to_act(P, feat), [L], offs, pos=tdev.data_ptr(), pos_period=table.shape[0])
    else:
        out = P.encoder(T.to_act(P, feat), [L], offs, pos=T.to_act(P, pos).ptr)
    desc = P.ops[-1][2]
    assert desc.dtype != 0
    if one_wave:
        assert desc.n_qtiles64 >= 512 and desc.n_qtiles192 > 0
        desc.n_qtiles192 = 0
    return desc, out


def _offs(length, hw):
    offs = [0]
    for n in length:
        offs.append(offs[-1] + n * hw[0] * hw[1])
    return offs


def _cases(T, timing=False):
    """-> (name, precision, d, sd, feat, offs, pos, table, one_wave)"""
    def shaped(name, precision, d, length, hw, period, one_wave=False):
        S, tag = sum(length), "ab" + name
        sd = T._encoder_sd(d, 192, tag)
        feat = T._rand((S, d) + hw, "f" + tag)
        pos = None if period else T._rand((S, d) + hw, "p" + tag, 0.5)
        table = None
        if period:  # [period, cs] rows: the real channels of a seeded table, pad channels zero
            table = torch.zeros(period, (d + 15) // 16 * 16)
            table[:, :d] = T._rand((period, d), "t" + tag, 0.5)
        return (name + ("_one_wave" if one_wave else ""), precision, d, sd, feat, _offs(length, hw), pos, table, one_wave)

    big = [shaped("cfg3", "bf16", 96, [1] * 57, (32, 24), 768), shaped("cfg5", "fp16", 78, [12], (24, 18), 0)]
    if timing:
        return big + [shaped("cfg3", "bf16", 96, [1] * 57, (32, 24), 768, one_wave=True)]
    out = []
    for case in sorted(T._LONG_GROUP_CASES):
        hw, length = T._LONG_GROUP_CASES[case]
        for d in (96, 78):
            sd, feat, pos, _ = T._long_group_case(case, d)
            for precision in ("bf16", "fp16"):
                for one_wave in (False, True):
                    out.append(("long_%s_%d_%s%s" % (case, d, precision, "_one_wave" if one_wave else ""), precision, d, sd, feat,
                                _offs(length, hw), pos, None, one_wave))
    marks = [m for m in T.test_encoder_layer_low_precision.pytestmark if m.name == "parametrize" and m.args[0].startswith("d,length")]
    for i, (d, length, hw, period) in enumerate(marks[0].args[1]):
        for precision in ("bf16", "fp16"):
            out.append(shaped("test%d_%s" % (i, precision), precision, d, list(length), tuple(hw), period))
    return out + big


def _kv_tensors(P, desc):
    by_ptr = {t.data_ptr(): t for t in P.keep if torch.is_tensor(t)}
    return by_ptr[desc.kbuf], by_ptr[desc.vbuf]


def dump(path):
    T = _setup()
    from i2r_amd import engine
    bufs = {}
    for name, precision, d, sd, feat, offs, pos, table, one_wave in _cases(T):
        P = engine.Program(torch.device(T.DEV))
        desc, out = _layer(T, P, precision, d, sd, feat, offs, pos, table, one_wave)
        T.run(P)
        k, v = _kv_tensors(P, desc)
        bufs[name + "/k"], bufs[name + "/v"], bufs[name + "/out"] = k.cpu(), v.cpu(), out.t.cpu()
        print("%-28s out checksum %.6f" % (name, out.t.float().abs().mean().item()), flush=True)
    torch.save(bufs, path)
    print("%d buffers, %d floats -> %s" % (len(bufs), sum(t.numel() for t in bufs.values()), path))


def compare(a_path, b_path, out_path):
    a, b = torch.load(a_path), torch.load(b_path)
    assert sorted(a) == sorted(b)
    # (bit patterns: a K / V buffer holds 16-bit images behind a float tensor, where a NaN pattern would not equal itself)
    diff = [n for n in sorted(a) if not torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))]
    cases = sorted({n.split("/")[0] for n in a})
    res = dict(method="one dump process per library on the same seeded inputs; K buffer, V buffer and layer output of every case compared "
               "with torch.equal on the bit patterns", cases=len(cases), buffers=len(a), floats=sum(t.numel() for t in a.values()),
               different=len(diff), different_buffers=diff, case_names=cases)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "case_names"}))
    return 1 if diff else 0


def time_inputs(reps=20):
    T = _setup()
    from i2r_amd import engine
    for name, precision, d, sd, feat, offs, pos, table, one_wave in _cases(T, timing=True):
        P = engine.Program(torch.device(T.DEV))
        _layer(T, P, precision, d, sd, feat, offs, pos, table, one_wave)
        P.finalize()
        for _ in range(reps):
            P.run()
        torch.cuda.synchronize()
        print("timed", name, flush=True)


def times(out_path, csvs):
    """kernel_stats CSVs in the order parent, new, parent, new -> average per launch (us) per kernel instantiation, merged into out_path"""
    runs = []
    for path in csvs:
        rows = {}
        for r in csv.DictReader(open(path)):
            m = re.search(r"(enc_\w+_k<[^>]*>)", r["Name"])
            if m and m.group(1).split("<")[0] in KERNELS:
                rows[m.group(1)] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
        runs.append(rows)
    kernels = []
    for k in sorted(runs[0]):
        par, new = [runs[0][k][1], runs[2][k][1]], [runs[1][k][1], runs[3][k][1]]
        pm, nm, bar = sum(par) / 2, sum(new) / 2, abs(par[0] - par[1])
        kernels.append(dict(kernel=k, calls=runs[0][k][0], parent_us=[round(x, 3) for x in par], branch_us=[round(x, 3) for x in new],
                            parent_mean=round(pm, 3), branch_mean=round(nm, 3), bar_us=round(bar, 3), inside=bool(nm - pm <= bar)))
    res = json.load(open(out_path)) if os.path.exists(out_path) else {}
    res["times"] = dict(method="rocprofv3 --kernel-trace --stats, no counters, one process per run, order parent, new, parent, new; average per "
                        "launch in us. bar_us = |parent run 1 - parent run 2|; inside = mean(new) - mean(parent) <= bar_us",
                        inputs="config-3-shaped layer (57 crops x 768 tokens, d = 96, bf16: enc_layer_lp4_k), the same with n_qtiles192 = 0 "
                        "(enc_layer_lp_k, QF = 4), config-5-shaped layer (12 x 432 tokens in one group, d = 78, fp16: enc_layer_lp_k, QF = 1); "
                        "20 launches each", kernels=kernels)
    json.dump(res, open(out_path, "w"), indent=1)
    for k in kernels:
        print(k)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "dump":
        dump(sys.argv[2])
    elif mode == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    elif mode == "time":
        time_inputs()
    elif mode == "times":
        times(sys.argv[2], sys.argv[3:7])
    else:
        sys.exit(__doc__)
