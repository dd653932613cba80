// What every dataset class of the reference does with the decoded key points before it writes a result, on device:
//   i2r_pose_nms    per-person rescoring (lib/dataset/coco.py:384-396) + per-image OKS-NMS / soft-OKS-NMS (lib/nms/nms.py:75-181)
// One workgroup per image (images are independent).  A latency kernel: a few workgroups on 256 CUs; the aim is to keep the step off the
// host, not a roofline fraction.  Per image of P persons:
//   1. rescoring, fp32, joints added in ascending order, one division, one multiplication (bit-identical to the reference's float32)
//   2. rank by counting on the float64 product mean * box_score, which is what the reference sorts (P^2 compares; equal products: lower
//      crop index first)
//   3. the image's persons staged in LDS in rank order (SoA key points, area, visibility mask); beyond what fits they stay in global memory
//   4. hard form: the suppression relation as bit rows in LDS (P x ceil(P/64) 64-bit words, one __ballot per word, only the words at or
//      behind the row's own: a person only suppresses lower-ranked ones), then ONE wave sweeps the rows: OR of the kept rows' words
//      soft form: at most max_dets steps of (arg-max of the decayed scores, one OKS row, Gaussian decay)
// OKS: dx, dy, dx^2 + dy^2 in fp32 as the reference's float32 key points give them (no contraction), everything behind it in fp64.
#include <mutex>

#include "i2r_common.h"

namespace {

constexpr int NMS_NT = 1024;            // 16 waves: the P^2 J exp() of a crowded image spread over all four SIMDs
constexpr int NMS_MAX_PERSONS = 1024;   // bit rows of 1024 persons: 128 KB of the 160 KB LDS
constexpr size_t NMS_MAX_LDS = 150 * 1024;

__host__ __device__ inline size_t nms_lds_bytes(int pm, int J, int soft, bool stage) {
    const size_t head = soft ? (size_t)pm : (size_t)pm * (size_t)(pm >> 6);  // decayed scores | bit rows (8-byte units)
    return head * 8 + (size_t)pm * 16 + (stage ? (size_t)pm * J * 8 : 0);
}

template <bool STAGE>
__global__ __launch_bounds__(NMS_NT) void pose_nms_k(const i2r_pose_nms_args a, const int pm) {
    extern __shared__ unsigned long long sm64[];
    __shared__ double s_var[32];
    __shared__ double red_v[NMS_NT / 64];
    __shared__ int red_i[NMS_NT / 64], red_r[NMS_NT / 64];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.joints, W = pm >> 6;
    const int o0 = a.img_off[img], o1 = a.img_off[img + 1];
    const int P = o1 - o0;
    if (o0 < 0 || P < 0 || o1 > a.n_crops || P > a.max_persons) {  // offsets that do not describe this batch: nothing but the flag
        if (tid == 0) a.n_keep[img] = -1;
        return;
    }
    if (P == 0) {
        if (tid == 0) a.n_keep[img] = 0;
        return;
    }
    unsigned long long* bits = sm64;                  // hard form
    double* dsc = reinterpret_cast<double*>(sm64);    // soft form
    double* dkey = reinterpret_cast<double*>(sm64);   // both forms, until the ranking is done: the sort keys by crop index
    int* s_order = reinterpret_cast<int*>(sm64 + (a.soft ? (size_t)pm : (size_t)pm * W));
    float* s_area = reinterpret_cast<float*>(s_order + pm);
    unsigned* s_vis = reinterpret_cast<unsigned*>(s_area + pm);
    int* s_rank = reinterpret_cast<int*>(s_vis + pm);
    float* s_kx = reinterpret_cast<float*>(s_rank + pm);
    float* s_ky = s_kx + (size_t)J * pm;
    const float* gp = a.preds + (size_t)o0 * J * 2;
    const float* gm = a.maxvals + (size_t)o0 * J;

    if (tid < J) {
        const double s2 = 2.0 * (double)a.sigmas[tid];
        s_var[tid] = s2 * s2;
    }
    // 1. rescoring (coco.py:384-396)
    auto kpt_score = [&](int p) -> float {
        float sum = 0.f;
        int cnt = 0;
        for (int j = 0; j < J; ++j) {
            const float v = gm[(size_t)p * J + j];
            if ((double)v > a.in_vis_thre) {
                sum = __fadd_rn(sum, v);
                ++cnt;
            }
        }
        return cnt ? sum / (float)cnt : sum;
    };
    for (int p = tid; p < P; p += NMS_NT) {
        const float mean = kpt_score(p), box = a.box_score[o0 + p];
        a.score[o0 + p] = __fmul_rn(mean, box);
        // the sort key is the reference's float64 score: the product of two floats, exact in double (two persons whose scores round to
        // the same fp32 value are still ordered by value).  A NaN ranks last, so that the counting below is a permutation
        const double key = (double)mean * (double)box;
        dkey[p] = key == key ? key : -__builtin_inf();
    }
    __syncthreads();
    // 2. rank by counting: descending key, equal keys by ascending crop index
    for (int p = tid; p < P; p += NMS_NT) {
        const double sp = dkey[p];
        int pos = 0;
        for (int q = 0; q < P; ++q) {
            const double sq = dkey[q];
            pos += (sq > sp || (sq == sp && q < p)) ? 1 : 0;
        }
        s_order[pos] = p;
    }
    __syncthreads();
    // 3. stage in rank order
    const float vis_t = (float)a.oks_vis_thre;
    for (int r = tid; r < P; r += NMS_NT) {
        const int p = s_order[r];
        s_area[r] = a.area ? a.area[o0 + p]
                           : __fmul_rn(__fmul_rn(a.scale[(size_t)(o0 + p) * 2], 200.f), __fmul_rn(a.scale[(size_t)(o0 + p) * 2 + 1], 200.f));
        unsigned m = 0;
        for (int j = 0; j < J; ++j)
            if (!a.use_oks_vis || gm[(size_t)p * J + j] > vis_t) m |= 1u << j;
        s_vis[r] = m;
        s_rank[r] = -1;
        if (a.soft) dsc[r] = (double)kpt_score(p) * (double)a.box_score[o0 + p];  // the reference's float64 score: this product, exact
    }
    if (STAGE) {
        for (int i = tid; i < P * J; i += NMS_NT) {
            const int r = i / J, j = i - r * J;
            const float* kp = gp + ((size_t)s_order[r] * J + j) * 2;
            s_kx[(size_t)j * pm + r] = kp[0];
            s_ky[(size_t)j * pm + r] = kp[1];
        }
    }
    __syncthreads();

    // oks_iou (nms.py:75-98) of head g and candidate d, both rank positions; the joint mask is the CANDIDATE's alone (nms.py:95)
    auto oks = [&](int g, int d) -> double {
        const double den = ((double)s_area[g] + (double)s_area[d]) / 2.0 + 2.220446049250313e-16;  // np.spacing(1)
        const unsigned m = s_vis[d];
        const float* pg = gp + (size_t)s_order[g] * J * 2;
        const float* pd = gp + (size_t)s_order[d] * J * 2;
        double sum = 0.0;
        for (int j = 0; j < J; ++j) {
            float dx, dy;
            if (STAGE) {
                dx = __fsub_rn(s_kx[(size_t)j * pm + d], s_kx[(size_t)j * pm + g]);
                dy = __fsub_rn(s_ky[(size_t)j * pm + d], s_ky[(size_t)j * pm + g]);
            } else {
                dx = __fsub_rn(pd[2 * j], pg[2 * j]);
                dy = __fsub_rn(pd[2 * j + 1], pg[2 * j + 1]);
            }
            const double e = (double)__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) / s_var[j] / den / 2.0;
            if ((m >> j) & 1u) sum += exp(-e);
        }
        const int n = __popc(m);
        return n ? sum / (double)n : 0.0;
    };

    if (!a.soft) {
        // 4a. bit rows: bit c of row r = "r, if kept, suppresses c" (oks > thresh; <= keeps, nms.py:125)
        const int Wp = (P + 63) >> 6;
        for (int r = wave; r < P; r += NMS_NT / 64) {
            for (int w = r >> 6; w < Wp; ++w) {
                const int c = w * 64 + lane;
                bool sup = false;
                if (c > r && c < P) sup = oks(r, c) > a.oks_thre;
                const unsigned long long mword = __ballot(sup);
                if (lane == 0) bits[(size_t)r * W + w] = mword;
            }
        }
        __syncthreads();
        // 4b. greedy sweep by one wave: lane l holds word l of the suppressed set
        if (wave == 0) {
            unsigned long long removed = 0;
            int nk = 0;
            for (int r = 0; r < P; ++r) {
                const unsigned long long wd = __shfl(removed, r >> 6);
                if (!((wd >> (r & 63)) & 1ull)) {
                    if (lane >= (r >> 6) && lane < Wp) removed |= bits[(size_t)r * W + lane];
                    if (lane == 0) s_rank[r] = nk;
                    ++nk;
                }
            }
            if (lane == 0) a.n_keep[img] = nk;
        }
        __syncthreads();
    } else {
        // 4c. soft form (nms.py:142-181): take the head, decay the rest by exp(-oks^2 / thresh), re-sort (here: arg-max), stop at max_dets
        const int lim = (a.max_dets > 0 && a.max_dets < P) ? a.max_dets : P;
        for (int step = 0; step < lim; ++step) {
            double bv = -__builtin_inf();
            int bi = 0x7fffffff, br = -1;
            for (int r = tid; r < P; r += NMS_NT) {
                if (s_rank[r] >= 0) continue;
                const double v = dsc[r];
                const int i = s_order[r];
                if (br < 0 || v > bv || (v == bv && i < bi)) { bv = v; bi = i; br = r; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o), orr = __shfl_xor(br, o);
                if (orr >= 0 && (br < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; br = orr; }
            }
            if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_r[wave] = br; }
            __syncthreads();
            bv = red_v[0]; bi = red_i[0]; br = red_r[0];
            for (int k = 1; k < NMS_NT / 64; ++k) {
                const double ov = red_v[k];
                const int oi = red_i[k], orr = red_r[k];
                if (orr >= 0 && (br < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; br = orr; }
            }
            const int h = br;  // (never -1: step < P, so one person is left)
            if (tid == 0) s_rank[h] = step;  // (every scan of s_rank is behind the barrier above; the decay skips h itself)
            for (int r = tid; r < P; r += NMS_NT) {
                if (r == h || s_rank[r] >= 0) continue;
                const double ov = oks(h, r);
                dsc[r] = dsc[r] * exp(-(ov * ov) / a.oks_thre);
            }
            __syncthreads();
        }
        if (tid == 0) a.n_keep[img] = lim;
    }
    for (int r = tid; r < P; r += NMS_NT) a.rank[o0 + s_order[r]] = s_rank[r];
}

// kernels above 64 KB of dynamic LDS need the attribute, which is per device: set once per instance and device, to the most any
// launch asks for
template <bool STAGE>
hipError_t nms_allow_lds() {
    static std::mutex mu;
    static bool done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(pose_nms_k<STAGE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NMS_MAX_LDS);
        if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
    }
    return e;
}

}  // namespace

extern "C" int i2r_pose_nms(const i2r_pose_nms_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_pose_nms: null args");
    I2R_CHECK_ARG(a->n_crops >= 0 && a->n_img >= 0, "i2r_pose_nms: n_crops %d, n_img %d", a->n_crops, a->n_img);
    I2R_CHECK_ARG(a->joints >= 1 && a->joints <= 32, "i2r_pose_nms: %d joints (1..32)", a->joints);
    I2R_CHECK_ARG(a->max_persons >= 0 && a->max_persons <= NMS_MAX_PERSONS, "i2r_pose_nms: person count %d over the limit %d per image",
                  a->max_persons, NMS_MAX_PERSONS);
    I2R_CHECK_ARG(a->soft == 0 || a->soft == 1, "i2r_pose_nms: soft %d", a->soft);
    I2R_CHECK_ARG(a->oks_thre > 0.0, "i2r_pose_nms: oks_thre %g", a->oks_thre);
    if (a->n_crops == 0 || a->n_img == 0) return I2R_OK;
    I2R_CHECK_ARG(a->preds && a->maxvals && (a->scale || a->area) && a->box_score && a->img_off && a->sigmas, "i2r_pose_nms: null input pointer");
    I2R_CHECK_ARG(a->score && a->rank && a->n_keep, "i2r_pose_nms: null output pointer");
    I2R_CHECK_ARG(a->max_persons >= 1, "i2r_pose_nms: max_persons %d with %d crops", a->max_persons, a->n_crops);
    const int pm = (a->max_persons + 63) & ~63;
    const bool stage = nms_lds_bytes(pm, a->joints, a->soft, true) <= NMS_MAX_LDS;
    const size_t lds = nms_lds_bytes(pm, a->joints, a->soft, stage);
    I2R_CHECK_ARG(lds <= NMS_MAX_LDS, "i2r_pose_nms: %zu bytes of LDS", lds);
    auto k = stage ? pose_nms_k<true> : pose_nms_k<false>;
    if (lds > 64 * 1024) {
        const hipError_t e = stage ? nms_allow_lds<true>() : nms_allow_lds<false>();
        if (e != hipSuccess) {
            i2r_set_error("i2r_pose_nms: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
            return I2R_E_LAUNCH;
        }
    }
    i2r_launch(k, dim3((unsigned)a->n_img), dim3(NMS_NT), lds, (hipStream_t)stream, *a, pm);
    I2R_CHECK_LAUNCH("i2r_pose_nms");
    return I2R_OK;
}
