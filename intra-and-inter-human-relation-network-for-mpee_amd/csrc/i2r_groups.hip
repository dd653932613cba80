// Person groups of the reference's grouped test mode (PATCH_MODE main_target: lib/dataset/collater.py:28-51,164-173) on the device:
//   i2r_group_nearest   per person ("target") of an image the group [target, its k - 1 nearest other persons of the image], k = min(n, p)
// Distance: between the boxes' top-left corners, d = dx^2 + dy^2 in float64, every operation rounded on its own (no contraction) -- the
// argument of the square root np.linalg.norm takes; the order is by the key (d, person index), which is the reference's stable sort by
// distance wherever the square root keeps distinct d apart.  The target is always the first member (include/i2r_hip.h).
// One wave per target.  A latency kernel like i2r_pose_nms: the aim is to keep the step off the host.  Lanes stride over the image's
// persons; member q is the wave-wide arg-min over the keys strictly greater than member q - 1's key, so no "taken" state exists and
// any person count works.  No atomics, no LDS: two runs give the same table.
//   i2r_rows_gather_multi   the hand-over between the per-person and the per-group part of a grouped forward: up to 8 row gathers
// (pooled features, position rows, first-member features; both flip halves) by device tables in ONE launch.
#include <limits.h>
#include <string.h>

#include "i2r_common.h"

namespace {

constexpr int GN_WAVES = 4;  // targets per workgroup

#pragma clang fp contract(off)
__global__ __launch_bounds__(GN_WAVES * 64) void group_nearest_k(const double* __restrict__ anchors, const int* __restrict__ person_off,
                                                                  const int* __restrict__ member_off, int n_img, int n_persons,
                                                                  int n_members, int max_patch, int* __restrict__ members) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * GN_WAVES + (threadIdx.x >> 6);  // (wave-uniform: a whole wave leaves or stays)
    if (t >= n_persons) return;
    int lo = 0, hi = n_img - 1;  // the image of person t: the last b with person_off[b] <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (person_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const int s = person_off[lo], e = person_off[lo + 1];
    if (s < 0 || s > t || t >= e || e > n_persons) return;  // offsets that do not describe this batch: nothing is written
    const int n = e - s;
    const int k = n == 1 ? 1 : min(n, max_patch);
    const long long base = (long long)member_off[lo] + (long long)(t - s) * k;
    const long long end = min((long long)member_off[lo + 1], (long long)n_members);
    if (base < 0) return;
    if (lane == 0 && base < end) members[base] = t;
    const double tx = anchors[2 * (size_t)t], ty = anchors[2 * (size_t)t + 1];
    double pd = -1.0;  // key of the member found last; every d is >= 0
    int pj = -1;
    for (int q = 1; q < k; ++q) {
        double bd = 0.0;
        int bj = INT_MAX;  // INT_MAX: no candidate
        for (int j = s + lane; j < e; j += 64) {
            if (j == t) continue;
            const double dx = tx - anchors[2 * (size_t)j], dy = ty - anchors[2 * (size_t)j + 1];
            const double d = dx * dx + dy * dy;
            const bool behind = d > pd || (d == pd && j > pj);            // (a NaN distance is behind nothing: never a member)
            if (behind && (bj == INT_MAX || d < bd || (d == bd && j < bj))) { bd = d; bj = j; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {  // butterfly: every lane ends with the wave's minimum key
            const double od = __shfl_xor(bd, off);
            const int oj = __shfl_xor(bj, off);
            if (oj != INT_MAX && (bj == INT_MAX || od < bd || (od == bd && oj < bj))) { bd = od; bj = oj; }
        }
        if (lane == 0 && base + q < end) members[base + q] = bj == INT_MAX ? -1 : bj;
        if (bj == INT_MAX) continue;  // (non-finite anchors: the slots nobody qualifies for hold -1)
        pd = bd;
        pj = bj;
    }
}

// ---- i2r_rows_gather_multi ------------------------------------------------------------------------------------------------------
// A bandwidth kernel: whole rows of 16-byte chunks, nothing from LDS or the matrix pipe.  Flat 1-D grid; segment s owns the blocks
// [first[s], first[s + 1]), a row of it `bpr` consecutive blocks of `cpb` chunks each (the last one what is left), so a workgroup never
// straddles two rows: the segment scan, the table entry and its bound check are workgroup-uniform and read once (scalar loads).  The
// source address is formed only behind that check; a row whose entry is outside [0, n_src) is stored as zeros.  A lane moves up to
// GM_UNROLL chunks 256 apart (each wave-instruction 1 KiB contiguous), all loads issued before the first store.
constexpr int GM_THREADS = 256;
constexpr int GM_UNROLL = 4;
constexpr int GM_BLOCK_CHUNKS = GM_THREADS * GM_UNROLL;  // most chunks of a workgroup: 16 KiB

struct gm_seg {
    const f32x4* src;
    f32x4* out;
    const int* map;
    int n_src, chunks, bpr, cpb;  // chunks per row; blocks per row; chunks per block
};
struct gm_args {
    gm_seg seg[I2R_MAX_GATHER_SEGS];
    unsigned first[I2R_MAX_GATHER_SEGS + 1];  // block prefix: empty segments have first[s] == first[s + 1]
};

__global__ __launch_bounds__(GM_THREADS) void rows_gather_multi_k(const gm_args a) {
    const unsigned b = blockIdx.x;
    int s = 0;
#pragma unroll
    for (int i = 1; i < I2R_MAX_GATHER_SEGS; ++i) s += b >= a.first[i] ? 1 : 0;  // (uniform: no branch, no divergence)
    const gm_seg& g = a.seg[s];
    const unsigned local = b - a.first[s];
    const int row = (int)(local / (unsigned)g.bpr), part = (int)(local % (unsigned)g.bpr);
    const int c0 = part * g.cpb, c1 = min(c0 + g.cpb, g.chunks);
    const int m = g.map[row];
    const bool valid = (unsigned)m < (unsigned)g.n_src;  // (one compare: negative entries are huge as unsigned)
    f32x4* __restrict__ dst = g.out + (size_t)row * g.chunks;
    f32x4 v[GM_UNROLL];
#pragma unroll
    for (int i = 0; i < GM_UNROLL; ++i) v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const f32x4* __restrict__ srow = g.src + (size_t)m * g.chunks;
#pragma unroll
        for (int i = 0; i < GM_UNROLL; ++i) {
            const int c = c0 + (int)threadIdx.x + i * GM_THREADS;
            if (c < c1) v[i] = srow[c];
        }
    }
#pragma unroll
    for (int i = 0; i < GM_UNROLL; ++i) {
        const int c = c0 + (int)threadIdx.x + i * GM_THREADS;
        if (c < c1) dst[c] = v[i];
    }
}

}  // namespace

extern "C" int i2r_rows_gather_multi(const i2r_gather_multi_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_rows_gather_multi: null arguments");
    I2R_CHECK_ARG(a->n_seg >= 0 && a->n_seg <= I2R_MAX_GATHER_SEGS, "i2r_rows_gather_multi: n_seg=%d (0..%d)", a->n_seg, I2R_MAX_GATHER_SEGS);
    gm_args k;
    memset(&k, 0, sizeof(k));
    unsigned long long blocks = 0;
    for (int s = 0; s < I2R_MAX_GATHER_SEGS; ++s) {
        k.first[s] = (unsigned)blocks;
        k.seg[s].bpr = k.seg[s].cpb = 1;
        if (s >= a->n_seg) continue;
        const i2r_gather_seg& g = a->seg[s];
        I2R_CHECK_ARG(g.n_out >= 0, "i2r_rows_gather_multi: segment %d n_out=%d", s, g.n_out);
        if (g.n_out == 0) continue;
        I2R_CHECK_ARG(g.src && g.out && g.map && g.src != g.out, "i2r_rows_gather_multi: segment %d bad pointers", s);
        I2R_CHECK_ARG(g.n_src >= 0 && g.row_bytes > 0 && g.row_bytes % 16 == 0 && g.row_bytes / 16 <= 0x7fffffffll - GM_BLOCK_CHUNKS,
                      "i2r_rows_gather_multi: segment %d n_src=%d row_bytes=%lld (a positive multiple of 16)", s, g.n_src, (long long)g.row_bytes);
        I2R_CHECK_ARG((uintptr_t)g.src % 16 == 0 && (uintptr_t)g.out % 16 == 0, "i2r_rows_gather_multi: segment %d src / out not 16-byte aligned", s);
        gm_seg& o = k.seg[s];
        o.src = reinterpret_cast<const f32x4*>(g.src);
        o.out = reinterpret_cast<f32x4*>(g.out);
        o.map = g.map;
        o.n_src = g.n_src;
        o.chunks = (int)(g.row_bytes / 16);
        o.bpr = (o.chunks + GM_BLOCK_CHUNKS - 1) / GM_BLOCK_CHUNKS;
        o.cpb = (o.chunks + o.bpr - 1) / o.bpr;  // (even parts: a 4608-chunk row is 5 blocks of 922, not 4 of 1024 and one of 512)
        blocks += (unsigned long long)g.n_out * (unsigned)o.bpr;
        I2R_CHECK_ARG(blocks < (1ull << 31), "i2r_rows_gather_multi: grid");
    }
    k.first[I2R_MAX_GATHER_SEGS] = (unsigned)blocks;
    if (blocks == 0) return I2R_OK;
    i2r_launch(rows_gather_multi_k, dim3((unsigned)blocks), dim3(GM_THREADS), 0, (hipStream_t)stream, k);
    I2R_CHECK_LAUNCH("i2r_rows_gather_multi");
    return I2R_OK;
}

extern "C" int i2r_group_nearest(const double* anchors, const int32_t* person_off, const int32_t* member_off, int32_t n_img,
                                 int32_t n_persons, int32_t n_members, int32_t max_patch, int32_t* members, void* stream) {
    I2R_CHECK_ARG(max_patch >= 1 && max_patch <= 64, "i2r_group_nearest: max_patch %d (1..64)", max_patch);
    I2R_CHECK_ARG(n_img >= 0 && n_persons >= 0 && n_members >= 0, "i2r_group_nearest: n_img %d, n_persons %d, n_members %d", n_img, n_persons, n_members);
    if (n_persons == 0 || n_img == 0) return I2R_OK;
    I2R_CHECK_ARG(anchors && person_off && member_off && members, "i2r_group_nearest: null pointer");
    I2R_CHECK_ARG(n_members >= n_persons, "i2r_group_nearest: %d members for %d persons", n_members, n_persons);
    i2r_launch(group_nearest_k, dim3((unsigned)((n_persons + GN_WAVES - 1) / GN_WAVES)), dim3(GN_WAVES * 64), 0, (hipStream_t)stream, anchors,
               person_off, member_off, n_img, n_persons, n_members, max_patch, members);
    I2R_CHECK_LAUNCH("i2r_group_nearest");
    return I2R_OK;
}
