"""float64 reference of the attention per person (Engine.forward(..., persons=) / net.person_relations): a head-averaged [L, L] map P of an
inter-human group -- tests/_attn_ref.restate's, a float64 softmax(q k^T) of raw rows, or what the forward hooks got -- reduced over its
persons (L = persons * T, person p = tokens [p T, (p + 1) T)):
  dependency D[i, k] = (1 / T) sum_{q in i} P[q, k]      affect F[j, q] = sum_{k in j} P[q, k]      relation R[i, j] = (1 / T) sum_{q in i} F[j, q]
and, for the maps, torch's own F.interpolate(scale_factor=, mode="bilinear", align_corners=False) in float64 as tests/_attn_query_ref.py."""
import torch
import torch.nn.functional as F


def full_map(qk, heads, hp, k_off):
    """raw rows [L, >= k_off + heads hp] (q of head h at h hp, already scaled; k at k_off + h hp) -> float64 [L, L] head-averaged softmax"""
    q = qk.double()
    out = torch.zeros(q.shape[0], q.shape[0], dtype=torch.float64, device=q.device)
    for h in range(heads):
        out += torch.softmax(q[:, h * hp:(h + 1) * hp] @ q[:, k_off + h * hp:k_off + (h + 1) * hp].t(), dim=-1)
    return out / heads


def reduce_persons(full, T):
    """full [L, L], L = persons * T -> float64 (D [P, L], F [P, L], R [P, P] from F, R [P, P] from D)"""
    full = full.double()
    L = full.shape[0]
    assert full.shape == (L, L) and T >= 1 and L % T == 0
    P = L // T
    D = full.reshape(P, T, L).mean(1)
    Fm = full.reshape(L, P, T).sum(2).t().contiguous()
    return D, Fm, Fm.reshape(P, P, T).mean(2).t().contiguous(), D.reshape(P, P, T).sum(2)


def as_maps(rows, h, w, scale=1):
    """D or F [P, L] -> float64 [P, P, h * scale, w * scale]: row p read as P token maps [h, w], up-sampled as visualize.py does"""
    P, L = rows.shape
    assert L == P * h * w
    out = rows.double().reshape(P, P, h, w)
    if scale > 1:
        out = F.interpolate(out, scale_factor=scale, mode="bilinear", align_corners=False)
    return out
