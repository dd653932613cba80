// Multi-head softmax(q k^T) v over variable-length token groups: the attention core of nn.MultiheadAttention with MODEL.N_HEAD > 1
// (or of a pre-norm layer), for the DETR-style encoders of the reference (interformer_pureMulti.py:171-243, attention.py:37-112,
// transpose_h.py:168-240).  The fused single-head post-norm layer kernels (i2r_encoder.hip) cover every shipped yaml; this kernel is
// the general form behind the same config keys: the host composes a layer from 1x1 i2r_conv launches (q|k, v, out-proj, FFN),
// i2r_layernorm and this launch.
//
// One wave per (tile of 16 NQ queries of a group, head), flash-style over the group's keys in tiles of 16 (the next tile's operands
// fetched under the current one's arithmetic), everything on the fp32 matrix pipe
// (v_mfma_f32_16x16x4_f32) without LDS:
//   S^T = K Q^T     A = K rows (lane (li, g) holds key li, dims 16u + 4g + c as one 16-byte load), B = Q^T (same dims of query li):
//                   the contraction index of step (u, c) runs over g, i.e. over the four dims 16u + 4g + c -- any enumeration of the
//                   head's dims works as long as A and B agree, and this one makes both operands whole float4 loads;
//   D layout        lane (g, li) holds S^T[key 4g + r][query li], r < 4: the softmax statistics of query li live in lanes li + 16 g
//                   (two xor-shuffles), and p[r] IS the B operand of
//   O^T += V^T P^T  step r contracts over the keys 4g + r (A = V[key 4g + r][dim 16 db + li]); D = O^T[dim 16 db + 4g + r][query li],
//                   so the running rescale of query li never leaves the lane and the result is one float4 store per dim block.
// Head dims are padded to hp = a multiple of 16 by the host (zero weight rows: pad dims of q, k, v are exactly 0).
#include "i2r_common.h"

namespace {

struct MhK {
    const float* qk;   // [n_tok, qk_cs]: q of head h at channel h*hp, k at k_off + h*hp (q already scaled by head_dim^-0.5)
    const float* v;    // [n_tok, v_cs]
    float* out;        // [n_tok, out_cs]
    const int* grp_off;
    const int* key_len;  // optional: group g attends to its first key_len[g] rows only (the others are queries without being keys)
    int n_grp, heads, hp, k_off, qk_cs, v_cs, out_cs;
};

constexpr float kLog2e = 1.4426950408889634f;

template <int HB, int NQ>  // hp / 16, 16-query tiles per wave (they share every K / V fragment the wave loads)
__global__ __launch_bounds__(256) void enc_mh_attn_k(const MhK p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int head = blockIdx.y * (blockDim.x >> 6) + wave;
    if (head >= p.heads) return;  // (no barrier below)
    int t = blockIdx.x, gi = 0, g0 = 0, g1 = 0;
    for (; gi < p.n_grp; ++gi) {
        g0 = p.grp_off[gi];
        g1 = p.grp_off[gi + 1];
        const int nt = (g1 - g0 + 16 * NQ - 1) / (16 * NQ);
        if (t < nt) break;
        t -= nt;
    }
    if (gi >= p.n_grp) return;
    const int q0 = g0 + t * 16 * NQ;
    const int q1 = g1;                           // queries: the whole group
    if (p.key_len) g1 = g0 + min(max(p.key_len[gi], 1), g1 - g0);  // keys: its first key_len rows (key_padding_mask of the padded persons),
                                                                  // clamped to [1, group length]: no row of another group is ever read
    const int hc = head * p.hp + 4 * g;
    f32x4 q[NQ][HB], o[NQ][HB];
    float m[NQ], l[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const int qrow = min(q0 + 16 * n + li, q1 - 1);
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            q[n][u] = *reinterpret_cast<const f32x4*>(p.qk + (size_t)qrow * p.qk_cs + hc + 16 * u) * kLog2e;  // (exp2 below)
            o[n][u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        m[n] = -INFINITY;
        l[n] = 0.f;
    }
    // the operands of one key tile: K rows as float4 (lane: key li, dims 16u + 4g ..), V as the A operand of the PV steps (lane: dim li of
    // block db, key 4g + r); rows clamped to the group (their probabilities are zero)
    auto load_tile = [&](int k0, f32x4(&kk)[HB], float(&vv)[4][HB]) {
        const float* kp = p.qk + (size_t)min(k0 + li, g1 - 1) * p.qk_cs + p.k_off + hc;
#pragma unroll
        for (int u = 0; u < HB; ++u) kk[u] = *reinterpret_cast<const f32x4*>(kp + 16 * u);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* vp = p.v + (size_t)min(k0 + 4 * g + r, g1 - 1) * p.v_cs + head * p.hp + li;
#pragma unroll
            for (int db = 0; db < HB; ++db) vv[r][db] = vp[16 * db];
        }
    };
    f32x4 kk[HB], kn[HB];
    float vv[4][HB], vn[4][HB];
    load_tile(g0, kk, vv);
    for (int k0 = g0; k0 < g1; k0 += 16) {
        load_tile(min(k0 + 16, g1 - 1), kn, vn);  // (the next tile flies under this one's arithmetic; past the end: a harmless re-read)
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < HB; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) s = mfma16(kk[u][c], q[n][u][c], s);
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (k0 + 4 * g + r >= g1) s[r] = -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m[n], mx);  // (finite: key k0 of every tile exists)
            const float alpha = __builtin_amdgcn_exp2f(m[n] - m_new);
            float pr[4], ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pr[r] = __builtin_amdgcn_exp2f(s[r] - m_new);
                ps += pr[r];
            }
            l[n] = l[n] * alpha + ps;
            m[n] = m_new;
#pragma unroll
            for (int db = 0; db < HB; ++db) o[n][db] *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int db = 0; db < HB; ++db) o[n][db] = mfma16(vv[r][db], pr[r], o[n][db]);
        }
#pragma unroll
        for (int u = 0; u < HB; ++u) kk[u] = kn[u];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int db = 0; db < HB; ++db) vv[r][db] = vn[r][db];
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        float ls = l[n];
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        const float inv = 1.f / ls;
        if (q0 + 16 * n + li < q1) {
            float* op = p.out + (size_t)(q0 + 16 * n + li) * p.out_cs;
#pragma unroll
            for (int db = 0; db < HB; ++db) *reinterpret_cast<f32x4*>(op + hc + 16 * db) = o[n][db] * inv;
            // the columns behind the last head are the zero-weight pad columns of the out-proj: keep them finite
            if (head == 0)
                for (int c = p.heads * p.hp + 4 * g; c < p.out_cs; c += 16) *reinterpret_cast<f32x4*>(op + c) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
}

// crop i of out = crop map[i] of src, or zeros (map[i] < 0): the reference's padding_tensor (interformer.py:230-249) for the consumers that
// need the padded persons as ROWS (ATTENTION_TYPE window: their tokens are queries whose outputs the final view() redistributes)
__global__ __launch_bounds__(256) void rows_gather_k(const f32x4* __restrict__ src, f32x4* __restrict__ out, const int* __restrict__ map, int n_out, int per_crop4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_out * per_crop4) return;
    const int crop = (int)(i / per_crop4), r = (int)(i - (long long)crop * per_crop4);
    const int m = map[crop];
    out[i] = m >= 0 ? src[(size_t)m * per_crop4 + r] : (f32x4){0.f, 0.f, 0.f, 0.f};
}

// GeneralTransformerBlock.forward of attention.py (:1025-1029): the attention output [L, B, C] (L = P H W tokens of an image, B images) goes
// through permute(0, 2, 1).contiguous().view(B, C, P, H, W) -- a REINTERPRETATION of the [L, C, B] memory, not a transpose -- and
// permute(0, 2, 1, 3, 4).view(B P, C, H, W); get_valid_output then keeps the real persons.  Element (b', p', c', y, x) of the result is flat
// element f = (((b' C + c') P + p') H + y) W + x of [L, C, B], i.e. o[l = f / (C B)][b = f % B][c = (f / B) % C].  Restated as is.
// o: [B][L][cs] rows (image-major, as the attention launch writes them); out: NHWC crops of the real persons, crop s = (b', p') = pm[s].
__global__ __launch_bounds__(256) void view_scramble_k(const float* __restrict__ o, float* __restrict__ out, const int* __restrict__ pm, int n_out, int B, int P,
                                                        int C, int cs, int HW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_out * HW * cs) return;
    const int c = (int)(i % cs);
    const long long t = i / cs;
    const int yx = (int)(t % HW), s = (int)(t / HW);
    float v = 0.f;
    if (c < C) {
        const int bp = pm[s], b1 = bp / P, p1 = bp - b1 * P;
        const long long f = (((long long)b1 * C + c) * P + p1) * HW + yx;
        const int b = (int)(f % B);
        const long long r = f / B;
        const int cc = (int)(r % C);
        const long long l = r / C;
        v = o[((long long)b * P * HW + l) * cs + cc];
    }
    out[i] = v;
}

// ---- attention maps: the need_weights output of nn.MultiheadAttention (head-averaged softmax(q k^T)) --------------------------------
// Work item = (group, 16-query tile, block of kAwKeys keys), one wave each, four independent waves per workgroup.  Both passes walk the
// heads in order 0..heads-1 and the block's key tiles of 16, with the S^T = K Q^T fragment form of enc_mh_attn_k (lane (g, li) holds
// S^T[key 4g + r][query li], r < 4), fp32 matrix pipe, no LDS:
//   pass 1 (aw_stats_k)  per head: the running max m and the sum of exp2(s - m) of every query row over the block's keys -> ws
//   pass 2 (aw_probs_k)  per head: combine the row's block statistics into (M, 1 / L), recompute s, p = exp2(s - M) / L, add into the
//                        block's accumulators (fixed head order, no atomics); then one store per lane and key tile: 4 consecutive
//                        keys of one query row
// ws: per query row (token index) ws_stride floats = (m, l) per (key block, head).
// The query-point and per-person forms further down are these passes around other work items.  Every kernel of the family is a thin
// caller of the same pieces, so each piece of arithmetic exists once and the forms agree bit for bit:
//   aw_group        the walk over grp_off from a wave index to its group, with the workspace-stride guard
//   aw_block_stats  pass 1 of a 16-query tile over one key block (the online-softmax loop)
//   aw_row_stats    the combine: (M, 1 / L) of a row and head from its block statistics
//   aw_block_probs  pass 2 of a 16-query tile over the key tiles of one block, added into the caller's accumulators over the heads
//   aw_tile_probs   pass 2 of a 16-query tile against 16 key rows in the S = Q K^T form (the gathered columns, the roll-out's side 0)
//   aw_store4       the store tail: 4 consecutive floats of a row, one 16-byte piece or guarded elements
constexpr int kAwKeys = 128, kAwTiles = kAwKeys / 16;

struct AwK {
    const float* qk;
    float* out;
    const int* grp_off;
    const long long* out_off;
    float2* ws;
    int n_grp, heads, hp, k_off, qk_cs, ws_stride;
};

__host__ __device__ __forceinline__ int aw_key_blocks(int len) { return (len + kAwKeys - 1) / kAwKeys; }

// The group of wave `item` in a launch whose group gi (rows [g0, g1), len of them) has items(gi, len) work items; item becomes the index
// inside the group.  An empty group and one without items are skipped.  false past the last item, and for a group whose statistics do not
// fit a workspace row (compute nothing rather than overrun it).
template <class F>
__device__ __forceinline__ bool aw_group(const AwK& p, int& item, int& gi, int& g0, int& g1, F items) {
    for (gi = 0; gi < p.n_grp; ++gi) {
        g0 = p.grp_off[gi];
        g1 = p.grp_off[gi + 1];
        const int nt = g1 > g0 ? items(gi, g1 - g0) : 0;
        if (item < nt) return 2 * p.heads * aw_key_blocks(g1 - g0) <= p.ws_stride;
        item -= nt;
    }
    return false;
}

// the work item of wave `item`: group gi (rows [g0, g1)), query rows [q0, q0 + 16), key block kb of the group's nkb; false past the last one
__device__ __forceinline__ bool aw_item(const AwK& p, int item, int& gi, int& g0, int& g1, int& q0, int& kb, int& nkb) {
    if (!aw_group(p, item, gi, g0, g1, [](int, int len) { return (len + 15) / 16 * aw_key_blocks(len); })) return false;
    nkb = aw_key_blocks(g1 - g0);
    q0 = g0 + item / nkb * 16;
    kb = item - item / nkb * nkb;
    return true;
}

template <int HB>
__device__ __forceinline__ void aw_load_q(const AwK& p, int qrow, int head, int g, f32x4 (&q)[HB]) {
    const float* qp = p.qk + (size_t)qrow * p.qk_cs + head * p.hp + 4 * g;
#pragma unroll
    for (int u = 0; u < HB; ++u) q[u] = *reinterpret_cast<const f32x4*>(qp + 16 * u) * kLog2e;
}

template <int HB>
__device__ __forceinline__ f32x4 aw_scores(const AwK& p, int krow, int head, int g, const f32x4 (&q)[HB]) {
    const float* kp = p.qk + (size_t)krow * p.qk_cs + p.k_off + head * p.hp + 4 * g;
    f32x4 kk[HB];
#pragma unroll
    for (int u = 0; u < HB; ++u) kk[u] = *reinterpret_cast<const f32x4*>(kp + 16 * u);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < HB; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) s = mfma16(kk[u][c], q[u][c], s);
    return s;
}

// Block statistics: per head the running max m and the sum l of exp2(s - m) of query row qrow (lane (g, li): query li, keys 4g + r) over the
// keys [k_beg, k_end) of key block kb of its group (rows end at g1), online over tiles of 16 -> workspace row ws_row, if the lane's query
// is a valid one
template <int HB>
__device__ __forceinline__ void aw_block_stats(const AwK& p, int li, int g, int qrow, int g1, int k_beg, int k_end, bool valid, size_t ws_row, int kb) {
    for (int head = 0; head < p.heads; ++head) {
        f32x4 q[HB];
        aw_load_q<HB>(p, qrow, head, g, q);
        float m = -INFINITY, l = 0.f;
        for (int k0 = k_beg; k0 < k_end; k0 += 16) {
            f32x4 s = aw_scores<HB>(p, min(k0 + li, g1 - 1), head, g, q);
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (k0 + 4 * g + r >= k_end) s[r] = -INFINITY;
                mx = fmaxf(mx, s[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m, mx);  // (finite: key k0 of every tile exists)
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) ps += __builtin_amdgcn_exp2f(s[r] - m_new);
            l = l * __builtin_amdgcn_exp2f(m - m_new) + ps;
            m = m_new;
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        if (g == 0 && valid) p.ws[ws_row * (p.ws_stride / 2) + kb * p.heads + head] = make_float2(m, l);
    }
}

// The combine: (M, 1 / L) of one query row and head from the (m, l) of the row's nkb key blocks
__device__ __forceinline__ void aw_row_stats(const float2* st, int nkb, int heads, int head, float& mm, float& inv) {
    mm = -INFINITY;
    for (int b = 0; b < nkb; ++b) mm = fmaxf(mm, st[b * heads + head].x);
    float ll = 0.f;
    for (int b = 0; b < nkb; ++b) {
        const float2 e = st[b * heads + head];
        ll += e.y * __builtin_amdgcn_exp2f(e.x - mm);
    }
    inv = 1.f / ll;
}

// Block probabilities: acc[t][r] += exp2(s - M) / L of query row qrow (statistics row st) and key k_beg + 16 t + 4g + r, t < n_kt, over the
// heads in order; a lane that is not live (no query of its own) adds zeros
template <int HB, int TILES>
__device__ __forceinline__ void aw_block_probs(const AwK& p, int li, int g, int qrow, const float2* st, int nkb, bool live, int g1, int k_beg, int n_kt,
                                               f32x4 (&acc)[TILES]) {
    for (int head = 0; head < p.heads; ++head) {
        float mm, inv;
        aw_row_stats(st, nkb, p.heads, head, mm, inv);
        if (!live) inv = 0.f;
        f32x4 q[HB];
        aw_load_q<HB>(p, qrow, head, g, q);
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
            if (t < n_kt) {
                const f32x4 s = aw_scores<HB>(p, min(k_beg + 16 * t + li, g1 - 1), head, g, q);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][r] += __builtin_amdgcn_exp2f(s[r] - mm) * inv;
            }
        }
    }
}

// Tile probabilities in the S = Q K^T form (A = the rows of 16 queries, B = 16 key rows): acc[r] += exp2(s - M) / L of query row
// q0 + 4g + r (clamped to its group, which ends at g1) and the lane's key row krow, over the heads in order; lane (g, li) holds 4
// consecutive entries of column li, each with its own row's statistics
template <int HB>
__device__ __forceinline__ void aw_tile_probs(const AwK& p, int li, int g, int q0, int g1, int krow, int nkb, f32x4& acc) {
    const int hs2 = p.ws_stride / 2, qrow = min(q0 + li, g1 - 1);
    for (int head = 0; head < p.heads; ++head) {
        float mm[4], inv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)  // the statistics of the lane's 4 query rows
            aw_row_stats(p.ws + (size_t)min(q0 + 4 * g + r, g1 - 1) * hs2, nkb, p.heads, head, mm[r], inv[r]);
        f32x4 q[HB];
        aw_load_q<HB>(p, qrow, head, g, q);
        const float* kp = p.qk + (size_t)krow * p.qk_cs + p.k_off + head * p.hp + 4 * g;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < HB; ++u) {
            const f32x4 kk = *reinterpret_cast<const f32x4*>(kp + 16 * u);
#pragma unroll
            for (int c = 0; c < 4; ++c) s = mfma16(q[u][c], kk[c], s);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += __builtin_amdgcn_exp2f(s[r] - mm[r]) * inv[r];
    }
}

// The store tail: v = 4 consecutive floats of row `row` of the [*, len] block blk, at offset k (a multiple of 4) -- one 16-byte piece when the
// block is 16-byte aligned and 4 divides len (every piece then lies whole inside its row), guarded element stores otherwise: no store ever
// straddles a row end or touches a byte outside the block
__device__ __forceinline__ void aw_store4(float* blk, long long row, long long len, int k, f32x4 v) {
    if (k >= len) return;
    float* dst = blk + row * len + k;
    if ((len & 3) == 0 && (reinterpret_cast<uintptr_t>(blk) & 15) == 0) {
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (k + r < len) dst[r] = v[r];
    }
}

template <int HB>
__global__ __launch_bounds__(256) void aw_stats_k(const AwK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int gi, g0, g1, q0, kb, nkb;
    if (!aw_item(p, blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, q0, kb, nkb)) return;
    const int k_beg = g0 + kb * kAwKeys;
    aw_block_stats<HB>(p, li, g, min(q0 + li, g1 - 1), g1, k_beg, min(k_beg + kAwKeys, g1), q0 + li < g1, q0 + li, kb);
}

template <int HB>
__global__ __launch_bounds__(256) void aw_probs_k(const AwK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int gi, g0, g1, q0, kb, nkb;
    if (!aw_item(p, blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, q0, kb, nkb)) return;
    const int qrow = min(q0 + li, g1 - 1), k_beg = g0 + kb * kAwKeys, n_kt = (min(k_beg + kAwKeys, g1) - k_beg + 15) / 16;
    f32x4 acc[kAwTiles] = {};
    aw_block_probs<HB>(p, li, g, qrow, p.ws + (size_t)qrow * (p.ws_stride / 2), nkb, true, g1, k_beg, n_kt, acc);
    if (q0 + li >= g1) return;
    const float rh = 1.f / (float)p.heads;
    float* blk = p.out + p.out_off[gi];  // (read once: a load behind a store is not hoisted)
#pragma unroll
    for (int t = 0; t < kAwTiles; ++t)  // k: the first of the lane's 4 keys, relative to the group
        if (t < n_kt) aw_store4(blk, q0 + li - g0, g1 - g0, k_beg + 16 * t + 4 * g - g0, acc[t] * rh);
}

// ---- attention maps at query points: K rows (mode 0, "dependency") or K columns (mode 1, "affect") of the head-averaged map P ------------
// The visualisation reads P[q, :] or P[:, q] for a handful of tokens q per group; neither form ever builds [L, L].
//   mode 0  aq_row_stats_k / aq_rows_k: aw_block_stats / aw_block_probs with the QUERY side gathered -- work item (group, 16 gathered
//           queries, block of kAwKeys keys); workspace row = gi * K + k (K = row stride of q_tok), (m, l) per (key block, head) as above
//   mode 1  aw_stats_k unchanged (every row's statistics), then aq_cols_k: the KEY side gathered, S = Q K^T (A = query rows, B = gathered
//           key rows): lane (g, li) holds S[query 4g + r][gathered key li], i.e. 4 consecutive entries of column li -> one aw_store4
//           (aw_tile_probs: the family's second score form, its 4 rows' statistics from aw_row_stats)
//   aq_upsample_k: each [P_g, h, w] row -> [P_g, h scale, w scale], F.interpolate's bilinear align_corners=False arithmetic
// A negative token gives a zero row; a token >= L_g is clamped (the host validates; a device table cannot be checked by the entry point).
struct AqK {
    AwK a;
    const int* q_tok;
    const int* q_cnt;
    float* rows;  // scale > 1: the raw [K_g, L_g] rows of group g at rows + K * grp_off[g], up-sampled into out by aq_upsample_k
    int K, scale, h, w;
    int seg;  // > 0 (the per-person maps below): K_g = L_g / seg rows instead of q_cnt / K
};

__device__ __forceinline__ int aq_count(const AqK& p, int gi) { return p.q_cnt ? min(max(p.q_cnt[gi], 0), p.K) : p.K; }

// group gi's raw block: [K_g, L_g] row-major, in `out` (scale 1) or in the `rows` workspace
__device__ __forceinline__ float* aq_block(const AqK& p, int gi, int g0) {
    return p.scale > 1 ? p.rows + (long long)p.K * g0 : p.a.out + p.a.out_off[gi];
}

// mode 0 work item of wave `item`: group gi, gathered queries [k0q, k0q + 16) of its kq, key block kb of nkb
__device__ __forceinline__ bool aq_row_item(const AqK& p, int item, int& gi, int& g0, int& g1, int& k0q, int& kq, int& kb, int& nkb) {
    const auto items = [&](int grp, int len) { return ((kq = aq_count(p, grp)) + 15) / 16 * aw_key_blocks(len); };  // (kq: of the group the walk ends at)
    if (!aw_group(p.a, item, gi, g0, g1, items)) return false;
    nkb = aw_key_blocks(g1 - g0);
    k0q = item / nkb * 16;
    kb = item - item / nkb * nkb;
    return true;
}

template <int HB>
__global__ __launch_bounds__(256) void aq_row_stats_k(const AqK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int gi, g0, g1, k0q, kq, kb, nkb;
    if (!aq_row_item(p, blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, k0q, kq, kb, nkb)) return;
    const int tok = p.q_tok[(size_t)gi * p.K + min(k0q + li, kq - 1)];
    const int qrow = g0 + min(max(tok, 0), g1 - g0 - 1), k_beg = g0 + kb * kAwKeys;
    aw_block_stats<HB>(p.a, li, g, qrow, g1, k_beg, min(k_beg + kAwKeys, g1), k0q + li < kq, (size_t)gi * p.K + k0q + li, kb);
}

template <int HB>
__global__ __launch_bounds__(256) void aq_rows_k(const AqK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int gi, g0, g1, k0q, kq, kb, nkb;
    if (!aq_row_item(p, blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, k0q, kq, kb, nkb)) return;
    const int kr = min(k0q + li, kq - 1);
    const int tok = p.q_tok[(size_t)gi * p.K + kr];
    const int qrow = g0 + min(max(tok, 0), g1 - g0 - 1), k_beg = g0 + kb * kAwKeys, n_kt = (min(k_beg + kAwKeys, g1) - k_beg + 15) / 16;
    f32x4 acc[kAwTiles] = {};
    aw_block_probs<HB>(p.a, li, g, qrow, p.a.ws + ((size_t)gi * p.K + kr) * (p.a.ws_stride / 2), nkb, true, g1, k_beg, n_kt, acc);
    if (k0q + li >= kq) return;
    const float rh = tok < 0 ? 0.f : 1.f / (float)p.a.heads;  // (a skipped point: the row is written as zeros)
    float* blk = aq_block(p, gi, g0);
#pragma unroll
    for (int t = 0; t < kAwTiles; ++t)  // k: the first of the lane's 4 keys, relative to the group
        if (t < n_kt) aw_store4(blk, k0q + li, g1 - g0, k_beg + 16 * t + 4 * g - g0, acc[t] * rh);
}

// mode 1, behind aw_stats_k: work item (group, 16-query tile, 16 gathered keys), one wave each
template <int HB>
__global__ __launch_bounds__(256) void aq_cols_k(const AqK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, kq = 0;
    if (!aw_group(p.a, item, gi, g0, g1, [&](int grp, int len) { return (len + 15) / 16 * (((kq = aq_count(p, grp)) + 15) / 16); })) return;
    const int nkb = aw_key_blocks(g1 - g0), nkt = (kq + 15) / 16, q0 = g0 + item / nkt * 16, kt = item - item / nkt * nkt;
    const int kc = kt * 16 + li;  // the lane's column (as the B operand and as the owner of the results)
    const int tok = p.q_tok[(size_t)gi * p.K + min(kc, kq - 1)];
    const int krow = g0 + min(max(tok, 0), g1 - g0 - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    aw_tile_probs<HB>(p.a, li, g, q0, g1, krow, nkb, acc);
    if (kc >= kq) return;
    const float rh = tok < 0 ? 0.f : 1.f / (float)p.a.heads;
    aw_store4(aq_block(p, gi, g0), kc, g1 - g0, q0 - g0 + 4 * g, acc * rh);  // column kc as a contiguous vector over the query rows
}

// blockIdx.y = group; 4 consecutive floats of its [K_g, P_g, h scale, w scale] block per thread
__global__ __launch_bounds__(256) void aq_upsample_k(const AqK p) {
    const int gi = blockIdx.y;
    const int g0 = p.a.grp_off[gi], len = p.a.grp_off[gi + 1] - g0, hw = p.h * p.w, kq = p.seg > 0 ? len / p.seg : aq_count(p, gi);
    if (len <= 0 || len % hw != 0) return;  // (the entry point checks the host's copy of the table; never a partial map)
    const int H = p.h * p.scale, W = p.w * p.scale;
    const long long n = (long long)kq * len * p.scale * p.scale;
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    const float* src = p.rows + (long long)p.K * g0;  // [K_g * P_g][h][w]
    float* dst = p.a.out + p.a.out_off[gi];
    const float rs = 1.f / (float)p.scale;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long e = min(e0 + j, n - 1);
        const int ox = (int)(e % W), oy = (int)(e / W % H);
        const float* m = src + e / ((long long)W * H) * hw;
        const float sy = fmaxf(((float)oy + 0.5f) * rs - 0.5f, 0.f), sx = fmaxf(((float)ox + 0.5f) * rs - 0.5f, 0.f);
        const int y0 = (int)sy, x0 = (int)sx, y1 = min(y0 + 1, p.h - 1), x1 = min(x0 + 1, p.w - 1);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        v[j] = (1.f - ly) * ((1.f - lx) * m[y0 * p.w + x0] + lx * m[y0 * p.w + x1]) + ly * ((1.f - lx) * m[y1 * p.w + x0] + lx * m[y1 * p.w + x1]);
    }
    if (e0 + 4 <= n && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<f32x4*>(dst + e0) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) dst[e0 + j] = v[j];
    }
}

// ---- the flip test's maps: the mirrored pass's raw rows brought back into the plain frame, merged, up-sampled ------------------------------
// aq_upsample_k with two sources: M[r, p, y, x] = (a[r, p, y, x] + b[r, p, y, w - 1 - x]) / 2 (one rounded add, an exact halving), then the
// same align_corners=False arithmetic on M.  The rows of b were computed at the mirrored tokens (token_mirror_k), so only the map axis is
// left to un-mirror here.  scale 1 stores M itself.  No LDS, no atomics; nothing outside a computed block is written.
struct AfK {
    const float* a;
    const float* b;
    float* out;
    const int* grp_off;
    const long long* src_off;  // group g's raw [rows_g, L_g] block, the same offset in a and in b
    const long long* out_off;
    const int* q_cnt;
    int K, seg, scale, h, w;
};

// blockIdx.y = group; 4 consecutive floats of its [rows_g, P_g, h scale, w scale] block per thread
__global__ __launch_bounds__(256) void aq_flip_merge_k(const AfK p) {
    const int gi = blockIdx.y;
    const int g0 = p.grp_off[gi], len = p.grp_off[gi + 1] - g0, hw = p.h * p.w;
    if (len <= 0 || len % hw != 0 || (p.seg > 0 && len % p.seg != 0)) return;  // (the entry point checks the host's copy of the table)
    const int kq = p.seg > 0 ? len / p.seg : (p.q_cnt ? min(max(p.q_cnt[gi], 0), p.K) : p.K);
    const int H = p.h * p.scale, W = p.w * p.scale;
    const long long n = (long long)kq * len * p.scale * p.scale;
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= n) return;
    const float* sa = p.a + p.src_off[gi];  // [rows_g * P_g][h][w]
    const float* sb = p.b + p.src_off[gi];
    float* dst = p.out + p.out_off[gi];
    const float rs = 1.f / (float)p.scale;
    const int wm = p.w - 1;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long e = min(e0 + j, n - 1);
        const int ox = (int)(e % W), oy = (int)(e / W % H);
        const long long m0 = e / ((long long)W * H) * hw;
        const float* ma = sa + m0;
        const float* mb = sb + m0;
        const auto mg = [&](int y, int x) { return (ma[y * p.w + x] + mb[y * p.w + wm - x]) * 0.5f; };
        if (p.scale == 1) {
            v[j] = mg(oy, ox);
            continue;
        }
        const float sy = fmaxf(((float)oy + 0.5f) * rs - 0.5f, 0.f), sx = fmaxf(((float)ox + 0.5f) * rs - 0.5f, 0.f);
        const int y0 = (int)sy, x0 = (int)sx, y1 = min(y0 + 1, p.h - 1), x1 = min(x0 + 1, p.w - 1);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        v[j] = (1.f - ly) * ((1.f - lx) * mg(y0, x0) + lx * mg(y0, x1)) + ly * ((1.f - lx) * mg(y1, x0) + lx * mg(y1, x1));
    }
    if (e0 + 4 <= n && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<f32x4*>(dst + e0) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) dst[e0 + j] = v[j];
    }
}

// mu(t) = t - 2 (t mod w) + w - 1 for every entry of an int32 token table; a negative entry (a skip) stays as it is
__global__ __launch_bounds__(256) void token_mirror_k(const int* __restrict__ src, int* __restrict__ dst, long long n, int w) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int t = src[i];
    dst[i] = t < 0 ? t : t - 2 * (t % w) + w - 1;
}

// ---- attention per person: P reduced over the persons of an inter-human group (L_g = P_g seg tokens, person p = tokens [p seg, (p + 1) seg)) ----
//   F[j, q] = sum_{k in j} P[q, k]          ap_affect_k, behind aw_stats_k: work item (group, 16-query tile, person j), S^T = K Q^T as above;
//                                             aw_row_stats, then a sum of its own over j's keys (normalised once per head)
//   D[i, k] = (1 / seg) sum_{q in i} P[q, k]  ap_depend_k: work item (group, person i, block of kApKeys keys): aw_block_probs over ALL of i's
//                                             query tiles into one set of accumulators (narrower key blocks than kAwKeys keep the chip
//                                             filled), then a butterfly over the 16 query lanes
//   R[i, j] = (1 / seg) sum_{q in i} F[j, q]  ap_relation_k: one wave per (group, i, j), read back from F
// No [L, L] block: F and D are [P_g, L_g].  Fixed head, tile and lane orders, no atomics.  A person's end may lie inside a 16-key tile or a
// key block: the keys (F) or queries (D) past it are masked.  A group whose length seg does not divide is skipped (the host validates).
constexpr int kApKeys = 32, kApTiles = kApKeys / 16;

struct ApK {
    AwK a;  // a.out / a.out_off: the maps blocks (modes 1 and 2)
    float* rel;
    const long long* rel_off;
    float* rows;        // F of group g at rows + pmax * grp_off[g]; the raw D rows (mode 1, scale > 1) d_shift floats behind
    long long d_shift;
    int seg, mode, scale, pmax;
};

// group gi's raw [P_g, L_g] block of D (what = 1) or F (what = 2): the maps block where it is the mode's output at scale 1, else the workspace
__device__ __forceinline__ float* ap_block(const ApK& p, int what, int gi, int g0) {
    if (p.mode == what && p.scale == 1) return p.a.out + p.a.out_off[gi];
    return p.rows + (long long)p.pmax * g0 + (what == 1 ? p.d_shift : 0);
}

// work items per group of the three passes (L_g tokens, P_g persons); the host entry point counts with the same functions
__host__ __device__ __forceinline__ int ap_items(int pass, int len, int np) {
    return pass == 0 ? (len + 15) / 16 * np : pass == 1 ? np * ((len + kApKeys - 1) / kApKeys) : np * np;
}

// the group of wave `item` in pass `pass` and its np persons: false past the last one; item becomes the index inside the group
__device__ __forceinline__ bool ap_item(const ApK& p, int pass, int& item, int& gi, int& g0, int& g1, int& np) {
    if (!aw_group(p.a, item, gi, g0, g1, [&](int, int len) { return len % p.seg != 0 ? 0 : ap_items(pass, len, len / p.seg); })) return false;
    np = (g1 - g0) / p.seg;
    return true;
}

// F of one 16-query tile and one person: the share of query row qrow's attention (statistics row st) on the keys [k_beg, k_end), heads in
// order, each normalised once; the lane's part -- the caller adds the four key lanes (xor 16, 32) and divides by the heads
template <int HB>
__device__ __forceinline__ float ap_affect_part(const AwK& a, int li, int g, int qrow, const float2* st, int nkb, int k_beg, int k_end) {
    float acc = 0.f;
    for (int head = 0; head < a.heads; ++head) {
        float mm, inv;
        aw_row_stats(st, nkb, a.heads, head, mm, inv);
        f32x4 q[HB];
        aw_load_q<HB>(a, qrow, head, g, q);
        float hsum = 0.f;
        for (int k0 = k_beg; k0 < k_end; k0 += 16) {
            const f32x4 s = aw_scores<HB>(a, min(k0 + li, k_end - 1), head, g, q);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (k0 + 4 * g + r < k_end) hsum += __builtin_amdgcn_exp2f(s[r] - mm);
        }
        acc += hsum * inv;
    }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    return acc * (1.f / (float)a.heads);
}

// D of one person and one block of kApKeys keys: aw_block_probs of the queries [q_beg, q_end) over the keys [k_beg, k_end) of a group that
// ends at g1, tile after tile into one set of accumulators, a butterfly over the 16 query lanes, times rs -> row[k - g0]
template <int HB>
__device__ __forceinline__ void ap_depend_block(const AwK& a, int li, int g, int q_beg, int q_end, int g0, int g1, int k_beg, int k_end, float rs, float* row) {
    const int nkb = aw_key_blocks(g1 - g0), n_kt = (k_end - k_beg + 15) / 16;
    f32x4 acc[kApTiles] = {};
    for (int qt = q_beg; qt < q_end; qt += 16) {  // (a query lane past the person's end adds nothing)
        const int qrow = min(qt + li, q_end - 1);
        aw_block_probs<HB>(a, li, g, qrow, a.ws + (size_t)qrow * (a.ws_stride / 2), nkb, qt + li < q_end, g1, k_beg, n_kt, acc);
    }
#pragma unroll
    for (int t = 0; t < kApTiles; ++t) {
        f32x4 v = acc[t];
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // the 16 query lanes of key 4g + r, butterfly order
            v[r] += __shfl_xor(v[r], 1);
            v[r] += __shfl_xor(v[r], 2);
            v[r] += __shfl_xor(v[r], 4);
            v[r] += __shfl_xor(v[r], 8);
        }
        const int k = k_beg + 16 * t + 4 * g + li;  // lanes li < 4 store key 4g + li: 16 consecutive floats per tile
        if (t < n_kt && li < 4 && k < k_end) row[k - g0] = (li == 0 ? v[0] : li == 1 ? v[1] : li == 2 ? v[2] : v[3]) * rs;
    }
}

// one person's share of a row of F: the mean of seg consecutive floats, lane-strided partial sums and a butterfly over the wave
__device__ __forceinline__ float ap_mean(const float* f, int seg, int lane) {
    float s = 0.f;
    for (int t = lane; t < seg; t += 64) s += f[t];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
    return s / (float)seg;
}

template <int HB>
__global__ __launch_bounds__(256) void ap_affect_k(const ApK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, np;
    if (!ap_item(p, 0, item, gi, g0, g1, np)) return;
    const int q0 = g0 + item / np * 16, j = item - item / np * np, len = g1 - g0, nkb = aw_key_blocks(len);
    const int qrow = min(q0 + li, g1 - 1), k_beg = g0 + j * p.seg;
    const float f = ap_affect_part<HB>(p.a, li, g, qrow, p.a.ws + (size_t)qrow * (p.a.ws_stride / 2), nkb, k_beg, k_beg + p.seg);
    if (g == 0 && q0 + li < g1) ap_block(p, 2, gi, g0)[(long long)j * len + (q0 + li - g0)] = f;
}

template <int HB>
__global__ __launch_bounds__(256) void ap_depend_k(const ApK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, np;
    if (!ap_item(p, 1, item, gi, g0, g1, np)) return;
    const int len = g1 - g0, nb = (len + kApKeys - 1) / kApKeys, i = item / nb, kb = item - i * nb;
    const int k_beg = g0 + kb * kApKeys, q_beg = g0 + i * p.seg;
    ap_depend_block<HB>(p.a, li, g, q_beg, q_beg + p.seg, g0, g1, k_beg, min(k_beg + kApKeys, g1), 1.f / ((float)p.a.heads * (float)p.seg),
                        ap_block(p, 1, gi, g0) + (long long)i * len);
}

__global__ __launch_bounds__(256) void ap_relation_k(const ApK p) {
    const int lane = threadIdx.x & 63;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1, np;
    if (!ap_item(p, 2, item, gi, g0, g1, np)) return;
    const int i = item / np, j = item - i * np;
    const float r = ap_mean(ap_block(p, 2, gi, g0) + (long long)j * (g1 - g0) + (long long)i * p.seg, p.seg, lane);
    if (lane == 0) p.rel[p.rel_off[gi] + (long long)i * np + j] = r;
}

// ---- the target form of the maps per person: the grouped test mode keeps only member 0 (the target) of a group, so only ITS query rows ----
//   F_t[j, q] = F[j, q], q < seg      at_affect_k: work item (group, 16-query tile of the target, member j) -- ap_affect_part
//   D_t[k]    = D[0, k]               at_depend_k: work item (group, block of kApKeys keys) -- ap_depend_block over the target's queries
//   r[j]      = R[0, j]               at_relation_k: one wave per (group, j) -- ap_mean of F_t[j, :]
// behind at_stats_k, aw_block_stats on the target's query tiles only (workspace rows [g0, g0 + seg) of a group).  These are the i = 0 /
// q < seg work items of the person form through the same device functions in the same head, tile and lane orders: at scale 1 the outputs
// are bit-identical to row 0 of the person form.  A query lane past the target's end reads the target's last row and stores nothing.
// Compact workspace: F_t [m_g, seg] of group g at rows + grp_off[g]; the raw D_t [L_g] (mode 1, scale > 1) d_shift floats behind.
struct AtK {
    AwK a;  // a.out / a.out_off: the maps blocks (modes 1 and 2)
    float* rel;
    const long long* rel_off;
    float* rows;
    long long d_shift;
    int seg, mode, scale;
};

__device__ __forceinline__ float* at_block(const AtK& p, int what, int gi, int g0) {
    if (p.mode == what && p.scale == 1) return p.a.out + p.a.out_off[gi];
    return p.rows + g0 + (what == 1 ? p.d_shift : 0);
}

// work items per group of the four passes (statistics, F_t, D_t, r); the host entry point counts with the same function
__host__ __device__ __forceinline__ int at_items(int pass, int len, int seg) {
    return pass == 0 ? (seg + 15) / 16 * aw_key_blocks(len) : pass == 1 ? (seg + 15) / 16 * (len / seg) : pass == 2 ? (len + kApKeys - 1) / kApKeys : len / seg;
}

__device__ __forceinline__ bool at_item(const AtK& p, int pass, int& item, int& gi, int& g0, int& g1) {
    return aw_group(p.a, item, gi, g0, g1, [&](int, int len) { return len % p.seg != 0 ? 0 : at_items(pass, len, p.seg); });
}

template <int HB>
__global__ __launch_bounds__(256) void at_stats_k(const AtK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1;
    if (!at_item(p, 0, item, gi, g0, g1)) return;
    const int nkb = aw_key_blocks(g1 - g0), q0 = g0 + item / nkb * 16, kb = item - item / nkb * nkb, q_end = g0 + p.seg, k_beg = g0 + kb * kAwKeys;
    aw_block_stats<HB>(p.a, li, g, min(q0 + li, q_end - 1), g1, k_beg, min(k_beg + kAwKeys, g1), q0 + li < q_end, q0 + li, kb);
}

template <int HB>
__global__ __launch_bounds__(256) void at_affect_k(const AtK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1;
    if (!at_item(p, 1, item, gi, g0, g1)) return;
    const int np = (g1 - g0) / p.seg, q0 = g0 + item / np * 16, j = item - item / np * np, nkb = aw_key_blocks(g1 - g0), q_end = g0 + p.seg;
    const int qrow = min(q0 + li, q_end - 1), k_beg = g0 + j * p.seg;
    const float f = ap_affect_part<HB>(p.a, li, g, qrow, p.a.ws + (size_t)qrow * (p.a.ws_stride / 2), nkb, k_beg, k_beg + p.seg);
    if (g == 0 && q0 + li < q_end) at_block(p, 2, gi, g0)[(long long)j * p.seg + (q0 + li - g0)] = f;
}

template <int HB>
__global__ __launch_bounds__(256) void at_depend_k(const AtK p) {
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1;
    if (!at_item(p, 2, item, gi, g0, g1)) return;
    const int k_beg = g0 + item * kApKeys;
    ap_depend_block<HB>(p.a, li, g, g0, g0 + p.seg, g0, g1, k_beg, min(k_beg + kApKeys, g1), 1.f / ((float)p.a.heads * (float)p.seg), at_block(p, 1, gi, g0));
}

__global__ __launch_bounds__(256) void at_relation_k(const AtK p) {
    const int lane = threadIdx.x & 63;
    int item = blockIdx.x * 4 + (threadIdx.x >> 6), gi, g0, g1;
    if (!at_item(p, 3, item, gi, g0, g1)) return;
    const float r = ap_mean(at_block(p, 2, gi, g0) + (long long)item * p.seg, p.seg, lane);
    if (lane == 0) p.rel[p.rel_off[gi] + item] = r;
}

// ---- attention roll-out: one step X' = (1 - alpha) X + alpha X P (side 0) or (1 - alpha) X + alpha X P^T (side 1) of a thin matrix -----------
// X [K_g, L_g] per group, the scale-1 layout of the query maps.  Behind aw_stats_k (every row's statistics), one product pass, one workgroup
// of kArWaves waves per (group, 16 output columns, chunk of kArRows rows of X): wave w walks every kArWaves-th piece of the reduction
// dimension in ascending order, the partial sums meet in LDS and are added in wave order (a fixed-order combine: deterministic):
//   side 1 (ar_step_k<HB, 1>)  out[k, q] = sum_j X[k, j] P[q, j]: aw_block_probs of the 16 queries q over pieces of kApKeys keys
//                              (S^T form: lane (g, li) holds P[query li][key 4g + r]), and p[r] IS the B operand of step r against
//                              A = X[row li][keys 4g .. 4g + 3] -- the way enc_mh_attn_k feeds P into P V
//   side 0 (ar_step_k<HB, 0>)  out[k, j] = sum_q X[k, q] P[q, j]: aw_tile_probs of the 16 keys j against one 16-query tile after the
//                              other (S form: lane (g, li) holds P[query 4g + r][key li]), B of step r against A = X[row li][queries 4g ..]
// Either way lane (g, li) ends with out[row 4g + r][column li].  The probabilities are summed over the heads (fixed order) before the
// product; 1 / heads goes into the closing scale.  A key / query past the group's end has a clamped, finite probability and meets a zero
// of X (ar_load4 reads nothing outside the block).  LDS for the combine only (the operands stay in registers), no atomics.  The last step of a chain writes its raw rows into the `rows`
// workspace and aq_upsample_k makes the maps.
constexpr int kArRows = 64, kArTiles = kArRows / 16, kArWaves = 8;  // (kArWaves >= kArTiles: wave x closes row tile x)

struct ArK {
    AqK q;  // q.a.out / q.a.out_off: the output blocks; q.rows: the raw rows at scale > 1
    const float* in;
    const long long* x_off;
    float alpha;
};

__device__ __forceinline__ int ar_count(const ArK& p, int gi, int len) {
    return p.q.seg > 0 ? (len % p.q.seg == 0 ? len / p.q.seg : 0) : aq_count(p.q, gi);
}

// X[row][k .. k + 3] of the [rows, len] block blk as the A operand of 4 matrix steps; zeros past the block's rows or the row's end
__device__ __forceinline__ f32x4 ar_load4(const float* blk, int row, int rows, int len, int k) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= rows || k >= len) return v;
    const float* src = blk + (long long)row * len + k;
    if ((len & 3) == 0 && (reinterpret_cast<uintptr_t>(blk) & 15) == 0) return *reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (k + r < len) v[r] = src[r];
    return v;
}

template <int HB, int SIDE>
__global__ __launch_bounds__(64 * kArWaves) void ar_step_k(const ArK p) {
    __shared__ f32x4 part[kArWaves][kArTiles][64];
    const int lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    int item = blockIdx.x, gi, g0, g1, kq = 0;  // (one item per workgroup: every wave takes the same branches up to the barrier)
    const auto items = [&](int grp, int len) { return (len + 15) / 16 * (((kq = ar_count(p, grp, len)) + kArRows - 1) / kArRows); };
    if (!aw_group(p.q.a, item, gi, g0, g1, items)) return;
    const int len = g1 - g0, nkb = aw_key_blocks(len), nch = (kq + kArRows - 1) / kArRows;
    const int c0 = g0 + item / nch * 16, r0 = (item - item / nch * nch) * kArRows;  // the item's 16 output columns (tokens), its first row of X
    const float* xin = p.in + p.x_off[gi];
    f32x4 o[kArTiles] = {};
    if (SIDE == 1) {
        const int qrow = min(c0 + li, g1 - 1);
        const float2* st = p.q.a.ws + (size_t)qrow * (p.q.a.ws_stride / 2);
        for (int k_beg = g0 + wave * kApKeys; k_beg < g1; k_beg += kArWaves * kApKeys) {  // the wave's pieces of 32 keys, ascending
            const int n_kt = (min(k_beg + kApKeys, g1) - k_beg + 15) / 16;
            f32x4 acc[kApTiles] = {};
            aw_block_probs<HB>(p.q.a, li, g, qrow, st, nkb, c0 + li < g1, g1, k_beg, n_kt, acc);
#pragma unroll
            for (int t = 0; t < kApTiles; ++t) {
                if (t < n_kt) {
#pragma unroll
                    for (int x = 0; x < kArTiles; ++x) {
                        if (r0 + 16 * x < kq) {
                            const f32x4 xa = ar_load4(xin, r0 + 16 * x + li, kq, len, k_beg - g0 + 16 * t + 4 * g);
#pragma unroll
                            for (int r = 0; r < 4; ++r) o[x] = mfma16(xa[r], acc[t][r], o[x]);
                        }
                    }
                }
            }
        }
    } else {
        const int krow = min(c0 + li, g1 - 1);
        for (int qt = g0 + wave * 16; qt < g1; qt += kArWaves * 16) {  // the wave's query tiles, ascending
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            aw_tile_probs<HB>(p.q.a, li, g, qt, g1, krow, nkb, acc);
#pragma unroll
            for (int x = 0; x < kArTiles; ++x) {
                if (r0 + 16 * x < kq) {
                    const f32x4 xa = ar_load4(xin, r0 + 16 * x + li, kq, len, qt - g0 + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[x] = mfma16(xa[r], acc[r], o[x]);
                }
            }
        }
    }
#pragma unroll
    for (int x = 0; x < kArTiles; ++x) part[wave][x][lane] = o[x];
    __syncthreads();
    // the combine: wave x adds the kArWaves partial sums of row tile x in wave order and writes the tile
    if (wave >= kArTiles || r0 + 16 * wave >= kq || c0 + li >= g1) return;
    f32x4 sum = part[0][wave][lane];
#pragma unroll
    for (int w = 1; w < kArWaves; ++w) sum += part[w][wave][lane];
    const float keep = 1.f - p.alpha, mix = p.alpha / (float)p.q.a.heads;
    float* blk = aq_block(p.q, gi, g0);
    const int col = c0 - g0 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // 16 lanes: 16 consecutive floats of one row
        const int row = r0 + 16 * wave + 4 * g + r;
        if (row >= kq) continue;
        const float xv = xin[(long long)row * len + col];
        blk[(long long)row * len + col] = p.alpha == 0.f ? xv : keep * xv + mix * sum[r];
    }
}

// ---- host side: what the entry points share ----
#define I2R_AW_TABLE(K) {K<1>, K<2>, K<3>, K<4>, K<5>, K<6>, K<7>, K<8>, K<9>, K<10>, K<11>, K<12>, K<13>, K<14>, K<15>, K<16>}  // [hp / 16 - 1]

#define I2R_AW_TABLE2(K, S) {K<1, S>, K<2, S>, K<3, S>, K<4, S>, K<5, S>, K<6, S>, K<7, S>, K<8, S>, K<9, S>, K<10, S>, K<11, S>, K<12, S>, K<13, S>, K<14, S>, K<15, S>, K<16, S>}

int mh_check_heads(const char* who, int heads, int hp) {
    I2R_CHECK_ARG(heads > 0 && hp > 0 && hp % 16 == 0 && hp <= 256, "%s: heads=%d hp=%d (hp: multiple of 16, <= 256)", who, heads, hp);
    return I2R_OK;
}

// the fields the attention-map entry points read alike (a non-null, its own pointers checked by the caller)
template <class A>
int aw_check(const char* who, const A* a) {
    if (const int e = mh_check_heads(who, a->heads, a->hp)) return e;
    const int hs = a->heads * a->hp;
    I2R_CHECK_ARG(a->k_off >= hs && a->k_off % 4 == 0 && a->qk_cs >= a->k_off + hs && a->qk_cs % 4 == 0, "%s: row stride qk=%d (k at %d) for %d heads x %d", who,
                  a->qk_cs, a->k_off, a->heads, a->hp);
    I2R_CHECK_ARG(a->n_grp > 0 && a->ws_stride >= 2 * a->heads && a->ws_stride % 2 == 0, "%s: n_grp=%d ws_stride=%d", who, a->n_grp, a->ws_stride);
    I2R_CHECK_ARG(reinterpret_cast<uintptr_t>(a->qk) % 16 == 0 && reinterpret_cast<uintptr_t>(a->ws) % 8 == 0, "%s: alignment", who);
    return I2R_OK;
}

template <class A>
AwK aw_args(const A* a, float* out, const int64_t* out_off) {
    return AwK{a->qk, out, a->grp_off, reinterpret_cast<const long long*>(out_off), reinterpret_cast<float2*>(a->ws), a->n_grp, a->heads, a->hp,
               a->k_off, a->qk_cs, a->ws_stride};
}

}  // namespace

extern "C" int i2r_rows_gather(const float* src, float* out, const int32_t* map, int32_t n_out, int32_t floats_per_crop, void* stream) {
    I2R_CHECK_ARG(src && out && map && src != out, "i2r_rows_gather: bad pointers");
    I2R_CHECK_ARG(n_out > 0 && floats_per_crop > 0 && floats_per_crop % 4 == 0, "i2r_rows_gather: n_out=%d floats_per_crop=%d", n_out, floats_per_crop);
    const long long n4 = (long long)n_out * (floats_per_crop / 4);
    I2R_CHECK_ARG((n4 + 255) / 256 < (1ll << 31), "i2r_rows_gather: grid");
    i2r_launch(rows_gather_k, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(src),
                       reinterpret_cast<f32x4*>(out), map, n_out, floats_per_crop / 4);
    I2R_CHECK_LAUNCH("i2r_rows_gather");
    return I2R_OK;
}

extern "C" int i2r_view_scramble(const float* o, float* out, const int32_t* person_map, int32_t n_out, int32_t n_images, int32_t max_persons, int32_t c,
                                 int32_t cs, int32_t hw, void* stream) {
    I2R_CHECK_ARG(o && out && person_map && o != out, "i2r_view_scramble: bad pointers");
    I2R_CHECK_ARG(n_out > 0 && n_images > 0 && max_persons > 0 && c > 0 && c <= cs && hw > 0, "i2r_view_scramble: sizes");
    const long long n = (long long)n_out * hw * cs;
    I2R_CHECK_ARG((n + 255) / 256 < (1ll << 31) && (long long)n_images * max_persons * hw * cs < (1ll << 40), "i2r_view_scramble: grid");
    i2r_launch(view_scramble_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, o, out, person_map, n_out, n_images, max_persons, c, cs, hw);
    I2R_CHECK_LAUNCH("i2r_view_scramble");
    return I2R_OK;
}

// ---- what i2r_mh_attention launches for its arguments: ONE check and ONE rule, shared by the launcher and by the launch-nothing query
//      i2r_mh_attention_form (include/i2r_hip.h), so that what the query reports cannot drift from what runs ----
namespace {

struct MhForm {
    int hb, nq;      // enc_mh_attn_k<hb, nq>: hp / 16, 16-query tiles per wave
    unsigned gx, gy;  // grid: the query tiles of 16 nq rows, the workgroups over the heads
    unsigned block;  // threads: 64 per wave, one wave per head of the workgroup
};

int mh_select_form(const char* who, const i2r_mh_attn_args* a, MhForm& f) {
    I2R_CHECK_ARG(a && a->qk && a->v && a->out && a->grp_off, "%s: null pointer", who);
    if (const int e = mh_check_heads(who, a->heads, a->hp)) return e;
    const int hs = a->heads * a->hp;
    I2R_CHECK_ARG(a->k_off >= hs && a->k_off % 4 == 0 && a->qk_cs >= a->k_off + hs && a->v_cs >= hs && a->out_cs >= hs && a->qk_cs % 4 == 0 &&
                      a->v_cs % 4 == 0 && a->out_cs % 4 == 0,
                  "%s: row strides qk=%d (k at %d) v=%d out=%d for %d heads x %d", who, a->qk_cs, a->k_off, a->v_cs, a->out_cs, a->heads, a->hp);
    I2R_CHECK_ARG(a->n_grp > 0 && a->n_qtiles64 > 0 && a->n_qtiles64 <= a->n_qtiles32 && a->n_qtiles32 <= a->n_qtiles16 && a->n_qtiles16 < (1 << 30),
                  "%s: n_grp=%d n_qtiles16/32/64=%d/%d/%d", who, a->n_grp, a->n_qtiles16, a->n_qtiles32, a->n_qtiles64);
    // query tiles per wave (they share the K / V fragments a wave loads; registers: q and o are NQ x HB fragments): up to 64 queries for
    // heads of <= 32 dims, 32 up to 96 dims, 16 beyond -- but never so few waves that the chip's 1024 SIMDs go unfilled (an inter-human
    // stack over a few hundred tokens per image keeps 16-query tiles)
    constexpr long long kMinWaves = 4096;
    f.hb = a->hp / 16;
    f.nq = 1;
    int n_tiles = a->n_qtiles16;
    if (f.hb <= 2 && (long long)a->n_qtiles64 * a->heads >= kMinWaves) {
        f.nq = 4;
        n_tiles = a->n_qtiles64;
    } else if (f.hb <= 6 && (long long)a->n_qtiles32 * a->heads >= kMinWaves) {
        f.nq = 2;
        n_tiles = a->n_qtiles32;
    }
    const int wpb = a->heads >= 4 ? 4 : a->heads;  // waves (= heads) per workgroup
    f.gx = (unsigned)n_tiles;
    f.gy = (unsigned)((a->heads + wpb - 1) / wpb);
    f.block = 64u * wpb;
    return I2R_OK;
}

}  // namespace

extern "C" int i2r_mh_attention_form(const i2r_mh_attn_args* a, int32_t* hb, int32_t* nq, int32_t* grid, int32_t* block) {
    I2R_CHECK_ARG(hb && nq, "i2r_mh_attention_form: null form pointer");
    MhForm f;
    if (const int e = mh_select_form("i2r_mh_attention_form", a, f)) return e;
    *hb = f.hb;
    *nq = f.nq;
    if (grid) {
        grid[0] = (int32_t)f.gx;
        grid[1] = (int32_t)f.gy;
    }
    if (block) *block = (int32_t)f.block;
    return I2R_OK;
}

extern "C" int i2r_mh_attention(const i2r_mh_attn_args* a, void* stream) {
    MhForm f;
    if (const int e = mh_select_form("i2r_mh_attention", a, f)) return e;
    MhK k{a->qk, a->v, a->out, a->grp_off, a->key_len, a->n_grp, a->heads, a->hp, a->k_off, a->qk_cs, a->v_cs, a->out_cs};
    typedef void (*fn_t)(const MhK);
    static const fn_t fn1[16] = {enc_mh_attn_k<1, 1>,  enc_mh_attn_k<2, 1>,  enc_mh_attn_k<3, 1>,  enc_mh_attn_k<4, 1>,  enc_mh_attn_k<5, 1>,  enc_mh_attn_k<6, 1>,
                                 enc_mh_attn_k<7, 1>,  enc_mh_attn_k<8, 1>,  enc_mh_attn_k<9, 1>,  enc_mh_attn_k<10, 1>, enc_mh_attn_k<11, 1>, enc_mh_attn_k<12, 1>,
                                 enc_mh_attn_k<13, 1>, enc_mh_attn_k<14, 1>, enc_mh_attn_k<15, 1>, enc_mh_attn_k<16, 1>};
    static const fn_t fn2[6] = {enc_mh_attn_k<1, 2>, enc_mh_attn_k<2, 2>, enc_mh_attn_k<3, 2>, enc_mh_attn_k<4, 2>, enc_mh_attn_k<5, 2>, enc_mh_attn_k<6, 2>};
    static const fn_t fn4[2] = {enc_mh_attn_k<1, 4>, enc_mh_attn_k<2, 4>};
    const fn_t fn = f.nq == 4 ? fn4[f.hb - 1] : f.nq == 2 ? fn2[f.hb - 1] : fn1[f.hb - 1];
    i2r_launch(fn, dim3(f.gx, f.gy), dim3(f.block), 0, (hipStream_t)stream, k);
    I2R_CHECK_LAUNCH("i2r_mh_attention");
    return I2R_OK;
}

extern "C" int i2r_attn_weights(const i2r_attn_weights_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->qk && a->out && a->grp_off && a->out_off && a->ws, "i2r_attn_weights: null pointer");
    if (const int e = aw_check("i2r_attn_weights", a)) return e;
    I2R_CHECK_ARG(a->n_tiles > 0, "i2r_attn_weights: n_tiles=%d", a->n_tiles);
    const AwK k = aw_args(a, a->out, a->out_off);
    typedef void (*fn_t)(const AwK);
    static const fn_t stats[16] = I2R_AW_TABLE(aw_stats_k);
    static const fn_t probs[16] = I2R_AW_TABLE(aw_probs_k);
    const dim3 grid((unsigned)((a->n_tiles + 3) / 4));
    i2r_launch(stats[a->hp / 16 - 1], grid, dim3(256), 0, (hipStream_t)stream, k);
    I2R_CHECK_LAUNCH("i2r_attn_weights (statistics)");
    i2r_launch(probs[a->hp / 16 - 1], grid, dim3(256), 0, (hipStream_t)stream, k);
    I2R_CHECK_LAUNCH("i2r_attn_weights (probabilities)");
    return I2R_OK;
}

extern "C" int i2r_attn_query_maps(const i2r_attn_query_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->qk && a->out && a->grp_off && a->out_off && a->ws && a->q_tok, "i2r_attn_query_maps: null pointer");
    I2R_CHECK_ARG(a->mode == 0 || a->mode == 1, "i2r_attn_query_maps: mode=%d (0: dependency rows, 1: affect columns)", a->mode);
    I2R_CHECK_ARG(a->scale >= 1 && a->scale <= 64, "i2r_attn_query_maps: scale=%d (1 .. 64)", a->scale);
    I2R_CHECK_ARG(a->K >= 1 && a->K < (1 << 20), "i2r_attn_query_maps: K=%d", a->K);
    if (const int e = aw_check("i2r_attn_query_maps", a)) return e;
    I2R_CHECK_ARG(a->n_grp < 65536 && a->n_tiles > 0 && (a->mode == 0 || a->n_col_tiles > 0), "i2r_attn_query_maps: n_grp=%d n_tiles=%d n_col_tiles=%d",
                  a->n_grp, a->n_tiles, a->n_col_tiles);
    int max_len = 0;
    if (a->scale > 1) {
        I2R_CHECK_ARG(a->rows && a->grp_off_host, "i2r_attn_query_maps: null pointer (scale > 1 needs rows and grp_off_host)");
        I2R_CHECK_ARG(a->h > 0 && a->w > 0 && (long long)a->h * a->w < (1 << 24), "i2r_attn_query_maps: h=%d w=%d", a->h, a->w);
        for (int g = 0; g < a->n_grp; ++g) {
            const int len = a->grp_off_host[g + 1] - a->grp_off_host[g];
            I2R_CHECK_ARG(len >= 0 && len % (a->h * a->w) == 0, /* (an empty group is skipped, as at scale 1) */ "i2r_attn_query_maps: group %d has %d tokens, not a multiple of h w = %d x %d", g, len, a->h, a->w);
            max_len = len > max_len ? len : max_len;
        }
    }
    const AqK k{aw_args(a, a->out, a->out_off), a->q_tok, a->q_cnt, a->rows, a->K, a->scale, a->h, a->w, 0};
    typedef void (*aw_t)(const AwK);
    typedef void (*aq_t)(const AqK);
    static const aw_t stats[16] = I2R_AW_TABLE(aw_stats_k);
    static const aq_t row_stats[16] = I2R_AW_TABLE(aq_row_stats_k);
    static const aq_t rows[16] = I2R_AW_TABLE(aq_rows_k);
    static const aq_t cols[16] = I2R_AW_TABLE(aq_cols_k);
    const int hb = a->hp / 16 - 1;
    const dim3 grid((unsigned)((a->n_tiles + 3) / 4));
    if (a->mode == 0) {
        i2r_launch(row_stats[hb], grid, dim3(256), 0, (hipStream_t)stream, k);
        I2R_CHECK_LAUNCH("i2r_attn_query_maps (row statistics)");
        i2r_launch(rows[hb], grid, dim3(256), 0, (hipStream_t)stream, k);
        I2R_CHECK_LAUNCH("i2r_attn_query_maps (rows)");
    } else {
        i2r_launch(stats[hb], grid, dim3(256), 0, (hipStream_t)stream, k.a);
        I2R_CHECK_LAUNCH("i2r_attn_query_maps (statistics)");
        i2r_launch(cols[hb], dim3((unsigned)((a->n_col_tiles + 3) / 4)), dim3(256), 0, (hipStream_t)stream, k);
        I2R_CHECK_LAUNCH("i2r_attn_query_maps (columns)");
    }
    if (a->scale > 1) {
        const long long n4 = ((long long)a->K * max_len * a->scale * a->scale + 3) / 4;
        I2R_CHECK_ARG((n4 + 255) / 256 < (1ll << 31), "i2r_attn_query_maps: up-sampling grid");
        if (n4 > 0)
            i2r_launch(aq_upsample_k, dim3((unsigned)((n4 + 255) / 256), (unsigned)a->n_grp), dim3(256), 0, (hipStream_t)stream, k);
        I2R_CHECK_LAUNCH("i2r_attn_query_maps (up-sampling)");
    }
    return I2R_OK;
}

extern "C" int i2r_attn_person_maps(const i2r_attn_person_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->qk && a->grp_off && a->ws && a->rel && a->rel_off && a->rows && a->grp_off_host, "i2r_attn_person_maps: null pointer");
    I2R_CHECK_ARG(a->mode >= 0 && a->mode <= 2, "i2r_attn_person_maps: mode=%d (0: relation only, 1: + dependency maps, 2: + affect maps)", a->mode);
    I2R_CHECK_ARG(a->mode == 0 || (a->maps && a->maps_off), "i2r_attn_person_maps: null pointer (modes 1 and 2 need maps and maps_off)");
    I2R_CHECK_ARG(a->scale >= 1 && a->scale <= 64, "i2r_attn_person_maps: scale=%d (1 .. 64)", a->scale);
    I2R_CHECK_ARG(a->seg >= 1 && a->seg < (1 << 24), "i2r_attn_person_maps: seg=%d", a->seg);
    if (const int e = aw_check("i2r_attn_person_maps", a)) return e;
    I2R_CHECK_ARG(a->n_grp < 65536, "i2r_attn_person_maps: n_grp=%d", a->n_grp);
    if (a->scale > 1)
        I2R_CHECK_ARG(a->h > 0 && a->w > 0 && (long long)a->h * a->w == a->seg, "i2r_attn_person_maps: seg=%d is not h w = %d x %d", a->seg, a->h, a->w);
    long long n_stats = 0, n_pass[3] = {0, 0, 0};
    int max_len = 0;
    for (int g = 0; g < a->n_grp; ++g) {
        const int len = a->grp_off_host[g + 1] - a->grp_off_host[g];
        I2R_CHECK_ARG(len >= 0 && len % a->seg == 0, /* (an empty group is skipped) */ "i2r_attn_person_maps: group %d has %d tokens, not a multiple of seg = %d", g, len, a->seg);
        if (len == 0) continue;
        n_stats += (long long)((len + 15) / 16) * aw_key_blocks(len);
        for (int pass = 0; pass < 3; ++pass) n_pass[pass] += ap_items(pass, len, len / a->seg);
        max_len = len > max_len ? len : max_len;
    }
    const int pmax = max_len / a->seg;
    I2R_CHECK_ARG(a->ws_stride >= 2 * a->heads * aw_key_blocks(max_len), "i2r_attn_person_maps: ws_stride=%d for %d heads and groups of up to %d tokens",
                  a->ws_stride, a->heads, max_len);
    I2R_CHECK_ARG(n_stats < (1ll << 31) && n_pass[0] < (1ll << 31) && n_pass[1] < (1ll << 31) && n_pass[2] < (1ll << 31), "i2r_attn_person_maps: grid");
    const long long n4 = ((long long)pmax * max_len * a->scale * a->scale + 3) / 4;
    I2R_CHECK_ARG((n4 + 255) / 256 < (1ll << 31), "i2r_attn_person_maps: up-sampling grid");
    if (max_len == 0) return I2R_OK;  // (every group is empty)
    const bool up = a->mode != 0 && a->scale > 1;
    const long long total = (long long)pmax * a->grp_off_host[a->n_grp];
    const ApK k{aw_args(a, a->maps, a->maps_off), a->rel, reinterpret_cast<const long long*>(a->rel_off), a->rows, total, a->seg, a->mode, up ? a->scale : 1, pmax};
    typedef void (*aw_t)(const AwK);
    typedef void (*ap_t)(const ApK);
    static const aw_t stats[16] = I2R_AW_TABLE(aw_stats_k);
    static const ap_t affect[16] = I2R_AW_TABLE(ap_affect_k);
    static const ap_t depend[16] = I2R_AW_TABLE(ap_depend_k);
    const int hb = a->hp / 16 - 1;
    const hipStream_t st = (hipStream_t)stream;
    i2r_launch(stats[hb], dim3((unsigned)((n_stats + 3) / 4)), dim3(256), 0, st, k.a);
    I2R_CHECK_LAUNCH("i2r_attn_person_maps (statistics)");
    i2r_launch(affect[hb], dim3((unsigned)((n_pass[0] + 3) / 4)), dim3(256), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_person_maps (affect)");
    if (a->mode == 1) {
        i2r_launch(depend[hb], dim3((unsigned)((n_pass[1] + 3) / 4)), dim3(256), 0, st, k);
        I2R_CHECK_LAUNCH("i2r_attn_person_maps (dependency)");
    }
    i2r_launch(ap_relation_k, dim3((unsigned)((n_pass[2] + 3) / 4)), dim3(256), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_person_maps (relation)");
    if (up) {  // the raw rows of the mode's maps (D behind F in the workspace) -> maps: the row layout of the query maps, K_g = P_g
        const AqK u{k.a, nullptr, nullptr, a->rows + (a->mode == 1 ? total : 0), pmax, a->scale, a->h, a->w, a->seg};
        i2r_launch(aq_upsample_k, dim3((unsigned)((n4 + 255) / 256), (unsigned)a->n_grp), dim3(256), 0, st, u);
        I2R_CHECK_LAUNCH("i2r_attn_person_maps (up-sampling)");
    }
    return I2R_OK;
}

extern "C" int i2r_attn_target_maps(const i2r_attn_target_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->qk && a->grp_off && a->ws && a->rel && a->rel_off && a->rows && a->grp_off_host, "i2r_attn_target_maps: null pointer");
    I2R_CHECK_ARG(a->mode >= 0 && a->mode <= 2, "i2r_attn_target_maps: mode=%d (0: relation only, 1: + dependency maps, 2: + affect maps)", a->mode);
    I2R_CHECK_ARG(a->mode == 0 || (a->maps && a->maps_off), "i2r_attn_target_maps: null pointer (modes 1 and 2 need maps and maps_off)");
    I2R_CHECK_ARG(a->scale >= 1 && a->scale <= 64, "i2r_attn_target_maps: scale=%d (1 .. 64)", a->scale);
    I2R_CHECK_ARG(a->seg >= 1 && a->seg < (1 << 24), "i2r_attn_target_maps: seg=%d", a->seg);
    if (const int e = aw_check("i2r_attn_target_maps", a)) return e;
    I2R_CHECK_ARG(a->n_grp < 65536, "i2r_attn_target_maps: n_grp=%d", a->n_grp);
    if (a->scale > 1)
        I2R_CHECK_ARG(a->h > 0 && a->w > 0 && (long long)a->h * a->w == a->seg, "i2r_attn_target_maps: seg=%d is not h w = %d x %d", a->seg, a->h, a->w);
    long long n_pass[4] = {0, 0, 0, 0};
    int max_len = 0;
    for (int g = 0; g < a->n_grp; ++g) {
        const int len = a->grp_off_host[g + 1] - a->grp_off_host[g];
        I2R_CHECK_ARG(len >= 0 && len % a->seg == 0, /* (an empty group is skipped) */ "i2r_attn_target_maps: group %d has %d tokens, not a multiple of seg = %d", g, len, a->seg);
        if (len == 0) continue;
        for (int pass = 0; pass < 4; ++pass) n_pass[pass] += at_items(pass, len, a->seg);
        max_len = len > max_len ? len : max_len;
    }
    I2R_CHECK_ARG(a->ws_stride >= 2 * a->heads * aw_key_blocks(max_len), "i2r_attn_target_maps: ws_stride=%d for %d heads and groups of up to %d tokens",
                  a->ws_stride, a->heads, max_len);
    I2R_CHECK_ARG(n_pass[0] < (1ll << 31) && n_pass[1] < (1ll << 31) && n_pass[2] < (1ll << 31) && n_pass[3] < (1ll << 31), "i2r_attn_target_maps: grid");
    const long long n4 = ((long long)max_len * a->scale * a->scale + 3) / 4;
    I2R_CHECK_ARG((n4 + 255) / 256 < (1ll << 31), "i2r_attn_target_maps: up-sampling grid");
    if (max_len == 0) return I2R_OK;  // (every group is empty)
    const bool up = a->mode != 0 && a->scale > 1;
    const long long total = a->grp_off_host[a->n_grp];
    const AtK k{aw_args(a, a->maps, a->maps_off), a->rel, reinterpret_cast<const long long*>(a->rel_off), a->rows, total, a->seg, a->mode, up ? a->scale : 1};
    typedef void (*at_t)(const AtK);
    static const at_t stats[16] = I2R_AW_TABLE(at_stats_k);
    static const at_t affect[16] = I2R_AW_TABLE(at_affect_k);
    static const at_t depend[16] = I2R_AW_TABLE(at_depend_k);
    const int hb = a->hp / 16 - 1;
    const hipStream_t st = (hipStream_t)stream;
    i2r_launch(stats[hb], dim3((unsigned)((n_pass[0] + 3) / 4)), dim3(256), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_target_maps (statistics)");
    i2r_launch(affect[hb], dim3((unsigned)((n_pass[1] + 3) / 4)), dim3(256), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_target_maps (affect)");
    if (a->mode == 1) {
        i2r_launch(depend[hb], dim3((unsigned)((n_pass[2] + 3) / 4)), dim3(256), 0, st, k);
        I2R_CHECK_LAUNCH("i2r_attn_target_maps (dependency)");
    }
    i2r_launch(at_relation_k, dim3((unsigned)((n_pass[3] + 3) / 4)), dim3(256), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_target_maps (relation)");
    if (up) {  // the raw row of the mode's maps (D_t behind F_t in the workspace) -> maps: one row of the query maps per group, K = 1
        const AqK u{k.a, nullptr, nullptr, a->rows + (a->mode == 1 ? total : 0), 1, a->scale, a->h, a->w, 0};
        i2r_launch(aq_upsample_k, dim3((unsigned)((n4 + 255) / 256), (unsigned)a->n_grp), dim3(256), 0, st, u);
        I2R_CHECK_LAUNCH("i2r_attn_target_maps (up-sampling)");
    }
    return I2R_OK;
}

extern "C" int i2r_attn_rollout_step(const i2r_attn_rollout_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->qk && a->in && a->out && a->grp_off && a->x_off && a->ws && a->grp_off_host, "i2r_attn_rollout_step: null pointer");
    I2R_CHECK_ARG(a->in != a->out, "i2r_attn_rollout_step: in == out (a step reads every row of in for every entry of out)");
    I2R_CHECK_ARG(a->side == 0 || a->side == 1, "i2r_attn_rollout_step: side=%d (0: X P, 1: X P^T)", a->side);
    I2R_CHECK_ARG(a->alpha >= 0.f && a->alpha <= 1.f, "i2r_attn_rollout_step: alpha=%g (0 .. 1)", (double)a->alpha);
    I2R_CHECK_ARG(a->scale >= 1 && a->scale <= 64, "i2r_attn_rollout_step: scale=%d (1 .. 64)", a->scale);
    I2R_CHECK_ARG(a->seg >= 0 && a->seg < (1 << 24) && (a->seg > 0 || (a->K >= 1 && a->K < (1 << 20))), "i2r_attn_rollout_step: seg=%d K=%d", a->seg, a->K);
    if (const int e = aw_check("i2r_attn_rollout_step", a)) return e;
    I2R_CHECK_ARG(a->n_grp < 65536, "i2r_attn_rollout_step: n_grp=%d", a->n_grp);
    if (a->scale > 1) {
        I2R_CHECK_ARG(a->rows && a->out_off && a->rows != a->in && a->rows != a->out, "i2r_attn_rollout_step: scale > 1 needs out_off and a rows workspace of its own");
        I2R_CHECK_ARG(a->h > 0 && a->w > 0 && (long long)a->h * a->w < (1 << 24), "i2r_attn_rollout_step: h=%d w=%d", a->h, a->w);
    }
    long long n_stats = 0, n_items = 0;
    int max_len = 0, max_rows = 0;
    for (int g = 0; g < a->n_grp; ++g) {
        const int len = a->grp_off_host[g + 1] - a->grp_off_host[g];
        I2R_CHECK_ARG(len >= 0 && (a->seg == 0 || len % a->seg == 0) && (a->scale == 1 || len % (a->h * a->w) == 0), /* (an empty group is skipped) */
                      "i2r_attn_rollout_step: group %d has %d tokens, not a multiple of seg = %d / h w = %d x %d", g, len, a->seg, a->h, a->w);
        if (len == 0) continue;
        const int rows = a->seg > 0 ? len / a->seg : a->K;  // (q_cnt lives on the device: K bounds it, surplus waves find no item)
        n_stats += (long long)((len + 15) / 16) * aw_key_blocks(len);
        n_items += (long long)((len + 15) / 16) * ((rows + kArRows - 1) / kArRows);  // (one workgroup each)
        max_len = len > max_len ? len : max_len;
        max_rows = rows > max_rows ? rows : max_rows;
    }
    I2R_CHECK_ARG(a->ws_stride >= 2 * a->heads * aw_key_blocks(max_len), "i2r_attn_rollout_step: ws_stride=%d for %d heads and groups of up to %d tokens",
                  a->ws_stride, a->heads, max_len);
    const long long n4 = ((long long)max_rows * max_len * a->scale * a->scale + 3) / 4;
    I2R_CHECK_ARG(n_stats < (1ll << 31) && n_items < (1ll << 31) && (n4 + 255) / 256 < (1ll << 31), "i2r_attn_rollout_step: grid");
    if (max_len == 0) return I2R_OK;  // (every group is empty)
    const int K = a->seg > 0 ? max_rows : a->K;  // the row stride of the rows workspace, as the up-sampling pass reads it
    const ArK k{AqK{aw_args(a, a->out, a->out_off ? a->out_off : a->x_off), nullptr, a->seg > 0 ? nullptr : a->q_cnt, a->rows, K, a->scale, a->h, a->w, a->seg},
                a->in, reinterpret_cast<const long long*>(a->x_off), a->alpha};
    typedef void (*aw_t)(const AwK);
    typedef void (*ar_t)(const ArK);
    static const aw_t stats[16] = I2R_AW_TABLE(aw_stats_k);
    static const ar_t step0[16] = I2R_AW_TABLE2(ar_step_k, 0);
    static const ar_t step1[16] = I2R_AW_TABLE2(ar_step_k, 1);
    const int hb = a->hp / 16 - 1;
    const hipStream_t st = (hipStream_t)stream;
    i2r_launch(stats[hb], dim3((unsigned)((n_stats + 3) / 4)), dim3(256), 0, st, k.q.a);
    I2R_CHECK_LAUNCH("i2r_attn_rollout_step (statistics)");
    i2r_launch((a->side ? step1 : step0)[hb], dim3((unsigned)n_items), dim3(64 * kArWaves), 0, st, k);
    I2R_CHECK_LAUNCH("i2r_attn_rollout_step (product)");
    if (a->scale > 1) {
        i2r_launch(aq_upsample_k, dim3((unsigned)((n4 + 255) / 256), (unsigned)a->n_grp), dim3(256), 0, st, k.q);
        I2R_CHECK_LAUNCH("i2r_attn_rollout_step (up-sampling)");
    }
    return I2R_OK;
}

extern "C" int i2r_attn_flip_merge(const i2r_attn_flip_merge_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->a && a->b && a->out && a->grp_off && a->src_off && a->out_off && a->grp_off_host, "i2r_attn_flip_merge: null pointer");
    I2R_CHECK_ARG(a->scale >= 1 && a->scale <= 64, "i2r_attn_flip_merge: scale=%d (1 .. 64)", a->scale);
    I2R_CHECK_ARG(a->h > 0 && a->w > 0 && (long long)a->h * a->w < (1 << 24), "i2r_attn_flip_merge: h=%d w=%d", a->h, a->w);
    I2R_CHECK_ARG(a->seg >= 0 && a->seg < (1 << 24) && (a->seg > 0 || (a->K >= 1 && a->K < (1 << 20))), "i2r_attn_flip_merge: seg=%d K=%d", a->seg, a->K);
    I2R_CHECK_ARG(a->n_grp > 0 && a->n_grp < 65536, "i2r_attn_flip_merge: n_grp=%d", a->n_grp);
    int max_len = 0, max_rows = 0;
    for (int g = 0; g < a->n_grp; ++g) {
        const int len = a->grp_off_host[g + 1] - a->grp_off_host[g];
        I2R_CHECK_ARG(len >= 0 && len % (a->h * a->w) == 0 && (a->seg == 0 || len % a->seg == 0), /* (an empty group is skipped) */
                      "i2r_attn_flip_merge: group %d has %d tokens, not a multiple of h w = %d x %d (seg = %d)", g, len, a->h, a->w, a->seg);
        max_len = len > max_len ? len : max_len;
        const int rows = a->seg > 0 ? len / a->seg : a->K;
        max_rows = rows > max_rows ? rows : max_rows;
    }
    const long long n4 = ((long long)max_rows * max_len * a->scale * a->scale + 3) / 4;
    I2R_CHECK_ARG((n4 + 255) / 256 < (1ll << 31), "i2r_attn_flip_merge: grid");
    if (n4 == 0) return I2R_OK;  // (every group is empty)
    const AfK k{a->a, a->b, a->out, a->grp_off, reinterpret_cast<const long long*>(a->src_off), reinterpret_cast<const long long*>(a->out_off),
                a->q_cnt, a->K, a->seg, a->scale, a->h, a->w};
    i2r_launch(aq_flip_merge_k, dim3((unsigned)((n4 + 255) / 256), (unsigned)a->n_grp), dim3(256), 0, (hipStream_t)stream, k);
    I2R_CHECK_LAUNCH("i2r_attn_flip_merge");
    return I2R_OK;
}

extern "C" int i2r_token_mirror(const int32_t* src, int32_t* dst, int64_t n, int32_t w, void* stream) {
    I2R_CHECK_ARG(src && dst, "i2r_token_mirror: null pointer");
    I2R_CHECK_ARG(n >= 0 && (n + 255) / 256 < (1ll << 31) && w >= 1, "i2r_token_mirror: n=%lld w=%d", (long long)n, w);
    if (n == 0) return I2R_OK;
    i2r_launch(token_mirror_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, (long long)n, w);
    I2R_CHECK_LAUNCH("i2r_token_mirror");
    return I2R_OK;
}
