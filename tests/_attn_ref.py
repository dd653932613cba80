"""CPU restatement of the attention maps the reference's forward hooks see (visualize.py:128-268,270-420): each encoder layer's input,
taken from the CPU oracle (oracle/i2r_cpu.forward(..., collect=)), through torch's own nn.MultiheadAttention arithmetic
(F.multi_head_attention_forward, need_weights=True: the head average) with the key-padding mask of the padded persons."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import i2r_cpu  # noqa: E402


def _tokens(f):  # [S, c, h, w] -> [S, h w, c]
    return f.flatten(2).transpose(1, 2)


def mha_weights(sd, p, t, n_head, key_mask=None):
    """t [B, L, d]: the q / k input of layer p (src + pos, or LN1(src) + pos) -> [B, L, L] head-averaged weights"""
    d = t.shape[-1]
    q = t.transpose(0, 1)
    _, w = F.multi_head_attention_forward(q, q, q, d, n_head, sd[p + ".self_attn.in_proj_weight"], sd[p + ".self_attn.in_proj_bias"],
                                          None, None, False, 0.0, sd[p + ".self_attn.out_proj.weight"], sd[p + ".self_attn.out_proj.bias"],
                                          training=False, key_padding_mask=key_mask, need_weights=True)
    return w


def _stack_maps(sd, stack, n_layers, inputs, pos, n_head, pre_norm, length=None):
    """inputs[l]: layer l's input tokens [S, T, c]; pos [S, T, c] or None.  length None: one batch entry per crop (intra-human),
    else per image with its persons' tokens (person, y, x) padded to max(length) and masked."""
    out = {}
    for l in range(n_layers):
        p = "%s.layers.%d" % (stack, l)
        src, ps, mask = inputs[l], pos, None
        if length is not None:
            S, T, c = src.shape
            B, N = len(length), max(length)
            src = i2r_cpu._pad_persons(src, length).reshape(B, N * T, c)
            ps = i2r_cpu._pad_persons(pos, length).reshape(B, N * T, c) if pos is not None else None
            mask = torch.zeros(B, N, T, dtype=torch.bool)
            for b, n in enumerate(length):
                mask[b, n:] = True
            mask = mask.view(B, N * T)
        t = F.layer_norm(src, (src.shape[-1],), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5) if pre_norm else src
        if ps is not None:
            t = t + ps
        out[(stack, l)] = mha_weights(sd, p, t, n_head, mask)
    return out


def restate(cfg, sd, x, pos_mask, length, standalone_single=False):
    """-> (maps {(stack, layer): [batch, L, L]}, inputs {stack: the stack's input features [S, c, h, w]}, oracle output)"""
    M = cfg["MODEL"]
    collect = {}
    with torch.no_grad():
        if standalone_single:
            y = i2r_cpu.forward_transpose_h(sd, "", cfg, x, collect)
        else:
            y = i2r_cpu.forward(sd, cfg, x, pos_mask, length, collect)
        maps, feats = {}, {}
        single = "" if standalone_single else "singleformer."
        if standalone_single or (M["NAME"] in ("interformer", "interformer_2stage") and M["SINGLEFORMER"] == "transpose_h"):
            ys = collect["stage3.%d" % (M["EXTRA"]["STAGE3"]["NUM_MODULES"] - 1)]
            f = F.conv2d(ys[M["HRNET_RES_LAYER"]], sd[single + "reduce.weight"])
            st = single + "global_encoder"
            feats[st] = f
            n = M["ENCODER_LAYERS"]
            ins = [_tokens(f)] + [collect["single.layers.%d" % l] for l in range(n - 1)]
            pos = sd[single + "pos_embedding"].reshape(1, -1, f.shape[1]).expand(f.shape[0], -1, -1) if M["POS_EMBEDDING"] != "none" else None
            maps.update(_stack_maps(sd, st, n, ins, pos, M["N_HEAD"], False))
        if standalone_single:
            return maps, feats, y
        if M["NAME"] == "interformer_pureMulti":
            st, n, f, pre = "global_encoder", M["ENCODER_LAYERS"], collect["reduce"], False
        else:
            st, n, pre = "multi_global_encoder", M["ENCODER_MULTI_LAYERS"], bool(M["NORMALIZE_BEFORE"]) and M["NAME"] == "interformer"
            if M["SINGLEFORMER"]:
                f = collect["single_feat"]
                for _ in range(int(math.log(f.shape[-1] // M["TRANS_SIZE"][-1], 2))):  # (the max-pool steps collect does not record)
                    f = i2r_cpu._maxpool(f)
            else:
                f = collect["reduce"]
        pos = collect.get("pos")
        if pos is not None and M["NAME"] == "interformer" and M["MULTI_POS_EMBEDDING"] == "cat_vec":
            f, pos = torch.cat([f, pos], dim=1), None
        feats[st] = f
        ins = [_tokens(f)] + [collect["%s.layers.%d" % (st, l)] for l in range(n - 1)]
        maps.update(_stack_maps(sd, st, n, ins, _tokens(pos) if pos is not None else None, M["N_HEAD"], pre, length))
    return maps, feats, y
