// Person groups of the reference's grouped test mode (PATCH_MODE main_target: lib/dataset/collater.py:28-51,164-173) on the device:
//   i2r_group_nearest   per person ("target") of an image the group [target, its k - 1 nearest other persons of the image], k = min(n, p)
// Distance: between the boxes' top-left corners, d = dx^2 + dy^2 in float64, every operation rounded on its own (no contraction) -- the
// argument of the square root np.linalg.norm takes; the order is by the key (d, person index), which is the reference's stable sort by
// distance wherever the square root keeps distinct d apart.  The target is always the first member (include/i2r_hip.h).
// One wave per target.  A latency kernel like i2r_pose_nms: the aim is to keep the step off the host.  Lanes stride over the image's
// persons; member q is the wave-wide arg-min over the keys strictly greater than member q - 1's key, so no "taken" state exists and
// any person count works.  No atomics, no LDS: two runs give the same table.
#include <limits.h>

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

}  // namespace

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
