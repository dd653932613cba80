"""float64 reference of the attention maps under the flip test (flip_maps="merged"), a restatement of the definitions of DESIGN.md
'i2r_attn_flip_merge' on top of tests/_attn_query_ref.py and tests/_attn_person_ref.py.  A stack group has tokens (p, y, x),
t = p h w + y w + x; the mirror is mu(p, y, x) = (p, y, w - 1 - x), mu(t) = t - 2 (t mod w) + w - 1, and a negative token (a skip) stays
negative.  With P the head-averaged map of the plain pass and P' the map of the same group in the mirrored pass:
  un-mirrored map  P~[q, k] = P'[mu(q), mu(k)]            merged map  M = (P + P~) / 2
  rows at token t  M[t, :]       columns  M[:, t]       (the mirrored pass is queried at mu(t), the other axis is un-mirrored)
  per person       R_m = (R + R') / 2,  D_m[i, k] = (D[i, k] + D'[i, mu(k)]) / 2,  F_m[j, q] = (F[j, q] + F'[j, mu(q)]) / 2
The merge happens on the raw token maps; up-sampling follows."""
import torch

from _attn_person_ref import as_maps, reduce_persons
from _attn_query_ref import query_maps


def mirror_tokens(tok, w):
    """mu of every entry of an integer tensor of tokens on token maps w wide; negatives are kept"""
    t = torch.as_tensor(tok).to(torch.int64)
    return torch.where(t < 0, t, t - 2 * (t % w) + w - 1)


def unmirror_map(full_m, w):
    """P' [L, L] of the mirrored pass -> P~[q, k] = P'[mu(q), mu(k)]"""
    mu = mirror_tokens(torch.arange(full_m.shape[0], device=full_m.device), w)
    return full_m.double()[mu][:, mu]


def merged_map(full, full_m, w):
    """M = (P + P~) / 2, float64 [L, L]"""
    return (full.double() + unmirror_map(full_m, w)) / 2


def unmirror_rows(rows_m, w):
    """rows [K, L] of the mirrored pass whose row index needs no un-mirroring (they were taken at mu(t), or belong to a whole person):
    the map axis brought back, out[r, k] = rows_m[r, mu(k)]"""
    mu = mirror_tokens(torch.arange(rows_m.shape[1], device=rows_m.device), w)
    return rows_m.double()[:, mu]


def merged_query_maps(full, full_m, tokens, mode, h, w, scale=1):
    """the query form: mode 0 the rows M[t, :], mode 1 the columns M[:, t] at tokens (negative: a zero map), as the decomposition computes
    them -- the plain pass at t, the mirrored pass at mu(t), its other axis un-mirrored, merged, THEN up-sampled
    -> float64 [K, persons, h scale, w scale]"""
    tok = torch.as_tensor(tokens).to(torch.int64)
    K, L = len(tok), full.shape[0]
    a = query_maps(full, tok, mode, h, w).reshape(K, L)
    b = query_maps(full_m, mirror_tokens(tok, w), mode, h, w).reshape(K, L)
    return as_query_maps((a + unmirror_rows(b, w)) / 2, h, w, scale)


def as_query_maps(rows, h, w, scale=1):
    """raw rows [K, persons h w] -> float64 [K, persons, h scale, w scale], up-sampled as tests/_attn_query_ref.py does"""
    K, L = rows.shape
    out = rows.double().reshape(K, L // (h * w), h, w)
    if scale > 1:
        out = torch.nn.functional.interpolate(out, scale_factor=scale, mode="bilinear", align_corners=False)
    return out


def merged_persons(full, full_m, h, w):
    """the per-person form from the two passes' own reductions -> float64 (D_m [P, L], F_m [P, L], R_m [P, P])"""
    D, F, R, _ = reduce_persons(full, h * w)
    Dm, Fm, Rm, _ = reduce_persons(full_m, h * w)
    return (D + unmirror_rows(Dm, w)) / 2, (F + unmirror_rows(Fm, w)) / 2, (R + Rm) / 2


__all__ = ["as_maps", "as_query_maps", "merged_map", "merged_persons", "merged_query_maps", "mirror_tokens", "unmirror_map", "unmirror_rows"]
