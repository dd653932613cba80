"""Generate the attention-map fixtures tests/golden/attn_<tag>.npz by running THE REFERENCE ITSELF on CPU (imported through
oracle/ref_shim.py, as oracle/make_golden.py does) with the hook recipe of its visualize.py (:128-268,270-420):

    model.<stack>.layers[i].self_attn.register_forward_hook(lambda m, i, o: maps.append(o[1]))

on the seeded synthetic weights and inputs of the existing golden cases.  Run in the build container only:

    python tools/make_golden_attn.py [tag ...]

Per tag, stack, layer and batch entry b it stores a few seeded query rows i of the [batch, L, L] output (full key width, the padded
columns included) -- keys  <stack>.<layer>.<b>.rows  (int64 row indices) and  <stack>.<layer>.<b>.maps  (fp32 [rows, L]) -- plus the
per-entry lengths  <stack>.lens  and the case's input checksums (tests/_golden.setup regenerates the inputs).  Data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import i2r_amd  # noqa: E402,F401
from i2r_amd import synth  # noqa: E402
import ref_shim  # noqa: E402
import _golden  # noqa: E402

TAGS = ["w48_l31", "tph_l21", "w48_nh8_l21", "hrt_pre_nh2_l21"]
STACKS = ("global_encoder", "multi_global_encoder", "singleformer.global_encoder")
ROWS = {"singleformer.global_encoder": 3}  # query rows per (layer, batch entry): 3 of 3072 for the intra-human stack, 8 elsewhere


def _get(mod, path):
    for p in path.split("."):
        mod = getattr(mod, p, None)
        if mod is None:
            return None
    return mod


def main():
    torch.set_num_threads(8)
    only = set(sys.argv[1:])
    for tag in TAGS:
        if only and tag not in only:
            continue
        cfg, sd, x, m, length, g = _golden.setup(tag)
        net = ref_shim.build_reference_model(cfg)
        net.load_state_dict(sd, strict=True)
        net.eval()
        maps, hooks = {}, []
        for st in STACKS:
            layers = _get(net, st + ".layers")
            if layers is None:
                continue
            for i in range(len(layers)):
                hooks.append(layers[i].self_attn.register_forward_hook(
                    lambda mod, inp, out, key=(st, i): maps.setdefault(key, []).append(out[1].detach().clone())))
        with torch.no_grad():
            net(x, m, length)
        for h in hooks:
            h.remove()
        data = dict(length=np.asarray(length, dtype=np.int64), x_checksum=g["x_checksum"])
        for (st, i), outs in sorted(maps.items()):
            assert len(outs) == 1, (st, i, len(outs))
            w = outs[0]  # [batch, L, L]
            tok = None
            if st == "singleformer.global_encoder":
                lens = [w.shape[1]] * w.shape[0]
            else:
                tok = w.shape[1] // max(length)
                lens = [n * tok for n in length]
            data["%s.lens" % st] = np.asarray(lens, dtype=np.int64)
            for b, n in enumerate(lens):
                k = ROWS.get(st, 8)
                rows = np.unique((synth.uniform01(7, "attn.%s.%s.%d.%d" % (tag, st, i, b), k) * n).astype(np.int64))
                data["%s.%d.%d.rows" % (st, i, b)] = rows
                data["%s.%d.%d.maps" % (st, i, b)] = w[b, torch.from_numpy(rows)].float().numpy()
                rs = w[b, :n, :n].double().sum(-1)
                print("%-16s %-28s layer %d entry %d: L %d of %d, row sums within %.1e of 1, padded keys max %.1e"
                      % (tag, st, i, b, n, w.shape[1], (rs - 1).abs().max().item(), w[b, :n, n:].abs().max().item() if n < w.shape[2] else 0.0))
        out = os.path.join(ROOT, "tests", "golden", "attn_%s.npz" % tag)
        np.savez_compressed(out, **data)
        print("%s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
