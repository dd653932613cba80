"""float64 reference of the attention maps at query points (Engine.forward(..., queries=) / net.attention_at): rows (mode 0) or columns
(mode 1) of a head-averaged [L, L] map -- tests/_attn_ref.restate's, or any other -- at token indices, each read as `persons` maps of
[h, w] and passed through torch's own F.interpolate(scale_factor=, mode="bilinear") in float64, as the reference's visualize.py does."""
import torch
import torch.nn.functional as F


def query_maps(full, tokens, mode, h, w, scale=1):
    """full [L, L] (L = persons * h * w); tokens: K indices, negative = skip (a zero map) -> float64 [K, persons, h * scale, w * scale]"""
    full = full.double()
    L = full.shape[0]
    assert full.shape == (L, L) and L % (h * w) == 0
    idx = torch.as_tensor(tokens, dtype=torch.int64, device=full.device)
    assert int(idx.max()) < L
    sel = full[idx.clamp(min=0)] if mode == 0 else full[:, idx.clamp(min=0)].t()
    sel = sel * (idx >= 0).to(sel.dtype)[:, None]
    out = sel.reshape(len(idx), L // (h * w), h, w)
    if scale > 1:
        out = F.interpolate(out, scale_factor=scale, mode="bilinear", align_corners=False)
    return out


def point_of_token(tok, fw, down):
    """a point (x, y) of the network input that lies inside token `tok` of a token map fw wide (the inverse of points_to_tokens)"""
    return [(tok % fw) * down + 0.25 * down, (tok // fw) * down + 0.75 * down]
