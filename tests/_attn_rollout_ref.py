"""float64 reference of the attention roll-out (i2r_attn_rollout_step / net.rollout_at / net.person_rollout).  With P_l the head-averaged
[L, L] map of captured layer l -- tests/_attn_person_ref.full_map of raw q|k rows, tests/_attn_ref.restate's, or what the forward hooks
got -- of the layers lo .. hi of one stack:
  A_l = (1 - alpha) I + alpha P_l        T = A_hi A_hi-1 ... A_lo        (rows sum to 1)
T is formed in float64 and read at the query tokens (rows: dependency, columns: affect) or reduced per person with
tests/_attn_person_ref.reduce_persons / as_maps.  chain() is the same product taken the way the kernel takes it, one thin step after the
other, in any dtype: the float32 form of it is the condition the raw cases must meet (tests/test_attn_rollout.py).
The raw cases of the GPU test live here, so that the CPU test checks the condition on exactly those inputs."""
import torch
import torch.nn.functional as F

from _attn_person_ref import as_maps, full_map, reduce_persons  # noqa: F401 (re-exported)

BAR = 1e-5  # per step: the bar single maps meet against float64 (tests/test_attn_maps_gpu.py TOL)

HEADS_HP = [(1, 96), (1, 80), (2, 48), (8, 16)]  # tests/test_attn_person_gpu.py
CHAINS = [(1, 0.5), (2, 1.0), (6, 0.5), (2, 0.0)]  # (steps, alpha)
# query cases: (group lengths, first token row, K, entries used per group or None); an empty group in the middle, lengths around the 16-key
# tile and the 128-key block, K around the 16-row tile and the 64-row chunk of the product pass
QUERY_LENS, QUERY_START = [1, 15, 17, 0, 127, 129, 257], 3
QUERY_K = [(1, None), (5, [5, 3, 5, 5, 1, 4, 5]), (17, None), (33, [33, 1, 17, 33, 16, 33, 32]), (70, [2, 70, 65, 0, 64, 70, 49])]
# person cases: (tokens per person, persons per group, first token row): a person boundary inside a 16-tile (12), inside a 128-key block
# (48), and more persons than one chunk of rows (1 x 70)
PERSON_CASES = [(12, [3, 0, 1], 3), (48, [3], 1), (1, [70, 0, 3], 2)]


def make_qk(heads, hp, n_tok, seed):
    """q|k rows as tests/test_attn_maps_gpu.py draws them (pad dims exactly 0, k behind a gap, a row stride with a tail), on the CPU, so
    that the CPU and the GPU tests see the same numbers -> (qk [n_tok, qk_cs], k_off, qk_cs)"""
    g = torch.Generator().manual_seed(seed)
    hd = hp - 3 if hp > 16 else hp
    hs = heads * hp
    k_off = hs + 16
    qk_cs = k_off + hs + 8
    qk = torch.zeros(n_tok, qk_cs)
    for h in range(heads):
        qk[:, h * hp:h * hp + hd] = torch.randn(n_tok, hd, generator=g) * 2.0 * hd ** -0.5
        qk[:, k_off + h * hp:k_off + h * hp + hd] = torch.randn(n_tok, hd, generator=g)
    return qk, k_off, qk_cs


def layer_seed(heads, hp, case, layer):
    return 7000 * heads + 13 * hp + 101 * case + layer


def query_tokens(K, lens, seed):
    """int32 [groups, K]: tokens inside each group, duplicates allowed, one negative entry (a skip) per group with K > 1"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.full((len(lens), K), -1, dtype=torch.int32)  # (an empty group: skips only)
    for i, n in enumerate(lens):
        if n:
            tok[i] = torch.randint(0, n, (K,), generator=g, dtype=torch.int32)
            tok[i, 0] = n - 1
            if K > 1:
                tok[i, (i + 1) % K] = -1
    return tok


def map_of(qk, heads, hp, k_off, dtype=torch.float64):
    """full_map in float64, or the same softmax taken in `dtype` (the float32 condition)"""
    if dtype == torch.float64:
        return full_map(qk, heads, hp, k_off)
    q = qk.to(dtype)
    out = torch.zeros(q.shape[0], q.shape[0], dtype=dtype, device=q.device)
    for h in range(heads):
        out += torch.softmax(q[:, h * hp:(h + 1) * hp] @ q[:, k_off + h * hp:k_off + (h + 1) * hp].t(), dim=-1)
    return out / heads


def rollout(maps, alpha):
    """maps: the [L, L] maps of layers lo .. hi, in that order -> float64 T = A_hi ... A_lo"""
    L = maps[0].shape[0]
    eye = torch.eye(L, dtype=torch.float64, device=maps[0].device)
    T = eye
    for P in maps:
        T = ((1 - alpha) * eye + alpha * P.double()) @ T
    return T


def seed_points(tokens, L, dtype=torch.float64):
    """one-hot rows [K, L] at the tokens; a negative token gives a zero row"""
    X = torch.zeros(len(tokens), L, dtype=dtype)
    for k, t in enumerate(tokens):
        if int(t) >= 0:
            X[k, int(t)] = 1
    return X


def seed_persons(n_pers, seg, side, dtype=torch.float64):
    """side 0 (dependency): row i = 1 / seg on person i's tokens; side 1 (affect): row j = 1 on person j's tokens"""
    X = torch.zeros(n_pers, n_pers * seg, dtype=dtype)
    for p in range(n_pers):
        X[p, p * seg:(p + 1) * seg] = 1.0 / seg if side == 0 else 1.0
    return X


def chain(X, maps, alpha, side):
    """the product as the kernel takes it: X' = (1 - alpha) X + alpha X P (side 0, layers hi -> lo) or alpha X P^T (side 1, lo -> hi), in
    the dtype of X; maps: layers lo .. hi in that order"""
    order = list(reversed(maps)) if side == 0 else list(maps)
    for P in order:
        P = P.to(X.dtype)
        X = (1 - alpha) * X + alpha * (X @ (P if side == 0 else P.t()))
    return X


def at_tokens(T, tokens, side):
    """rows (side 0) or columns (side 1) of T at the tokens, [K, L]; a negative token gives a zero row"""
    out = torch.zeros(len(tokens), T.shape[0], dtype=T.dtype, device=T.device)
    for k, t in enumerate(tokens):
        if int(t) >= 0:
            out[k] = T[int(t)] if side == 0 else T[:, int(t)]
    return out


def rows_as_maps(rows, h, w, scale=1):
    """[K, L] rows, L = P h w -> float64 [K, P, h scale, w scale], up-sampled as visualize.py does"""
    K, L = rows.shape
    out = rows.double().reshape(K, L // (h * w), h, w)
    if scale > 1:
        out = F.interpolate(out, scale_factor=scale, mode="bilinear", align_corners=False)
    return out


def relation_from(rows, seg, side):
    """R_T [P, P] from D_T (side 0: sum over person j's tokens) or from F_T (side 1: mean over person i's tokens, transposed)"""
    P = rows.shape[0]
    r = rows.reshape(P, P, seg)
    return r.sum(2) if side == 0 else r.mean(2).t()
