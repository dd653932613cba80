// Keypoint OKS evaluation on the device: what COCOeval(gt, dt, 'keypoints') does with the final poses (pycocotools cocoeval.py):
//   i2r_oks_match        computeOks + evaluateImg: one workgroup per image
//   i2r_oks_accumulate   accumulate: one workgroup per (group of images, area range, threshold)
// Latency kernels like i2r_pose_nms: the aim is to keep the step off the host.  All arithmetic is fp64 without contraction (__dmul_rn /
// __dadd_rn where a multiply feeds an add), no floating-point atomics: the discrete outputs are those of the numpy algorithm wherever
// its comparisons are not decided by the last ulp of exp(), and precision / recall are numpy's bits.
#include <mutex>

#include "i2r_common.h"

namespace {

constexpr int OKS_NT = 256;          // 4 waves: wave a walks area range a, lane t of it threshold t
constexpr int OKS_MAX_DETS = 32;
constexpr int OKS_MAX_GT = 256;
constexpr int OKS_MAX_DT = 1024;
constexpr int OKS_MAX_THR = 16;
constexpr int OKS_MAX_AREA = 4;
constexpr int OKS_MAX_REC = 128;
constexpr size_t OKS_MAX_LDS = (size_t)OKS_MAX_DETS * OKS_MAX_GT * 8;   // the [max_dets, G] OKS matrix: 64 KB (+ 11 KB static)
constexpr double OKS_EPS = 2.220446049250313e-16;                         // np.spacing(1)

__global__ __launch_bounds__(OKS_NT) void oks_match_k(const i2r_oks_match_args a) {
    extern __shared__ double s_oks[];                  // [nsel, G]: OKS of the detections that take part, score order
    __shared__ float s_sc[OKS_MAX_DT];                 // score by input index; NaN = the detection does not exist
    __shared__ double s_var[32], s_thr[OKS_MAX_THR], s_rng[2 * OKS_MAX_AREA], s_darea[OKS_MAX_DETS];
    __shared__ int s_sel[OKS_MAX_DETS];                // input index of the detection at score position r
    __shared__ unsigned s_gtm[OKS_MAX_AREA * OKS_MAX_THR * (OKS_MAX_GT / 32)];   // matched gts of every walk, bit rows
    __shared__ unsigned short s_walk[OKS_MAX_AREA][OKS_MAX_GT];                  // gt walk order per area range
    __shared__ unsigned char s_ig[OKS_MAX_AREA][OKS_MAX_GT], s_fl[OKS_MAX_GT];
    __shared__ int s_nvalid;
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int J = a.joints, nA = a.n_area, nT = a.n_thr;
    const int d0 = a.dt_off[img], d1 = a.dt_off[img + 1], g0 = a.gt_off[img], g1 = a.gt_off[img + 1];
    const int D = d1 - d0, G = g1 - g0;
    if (d0 < 0 || d1 < d0 || d1 > a.n_dt || D > a.max_dt_per_img || g0 < 0 || g1 < g0 || g1 > a.n_gt || G > a.max_gt_per_img) {
        const int lo = d0 > 0 ? d0 : 0, hi = d1 < a.n_dt ? d1 : a.n_dt;   // offsets that do not describe this batch: nothing but the flag
        for (int d = lo + tid; d < hi; d += OKS_NT) a.dt_rank[d] = -1;
        return;
    }
    if (tid < J) {
        const double s2 = a.sigmas[tid] * 2.0;
        s_var[tid] = s2 * s2;
    }
    if (tid < nT) s_thr[tid] = a.thr[tid];
    if (tid < 2 * nA) s_rng[tid] = a.area_rng[tid];
    if (tid == 0) s_nvalid = 0;
    for (int d = tid; d < D; d += OKS_NT) {
        float s = a.dt_score[d0 + d];
        if (s != s) s = -__builtin_inff();   // (a NaN score ranks last, so that the counting below is a permutation)
        s_sc[d] = (!a.dt_valid || a.dt_valid[d0 + d]) ? s : __builtin_nanf("");
    }
    for (int g = tid; g < G; g += OKS_NT) s_fl[g] = (unsigned char)(a.gt_flags[g0 + g] & 3);
    __syncthreads();

    // the image's OKS matrix of the optional output, if it lies inside the buffer
    long long ob = -1;
    if (a.oks) {
        const long long o = a.oks_off[img];
        if (o >= 0 && o + (long long)D * G <= a.oks_len) ob = o;
    }
    // 1. rank by counting: descending score, equal scores by ascending index
    int mine = 0;
    for (int d = tid; d < D; d += OKS_NT) {
        const float s = s_sc[d];
        int rank = -1;
        if (s == s) {
            ++mine;
            int pos = 0;
            for (int q = 0; q < D; ++q) {
                const float t = s_sc[q];   // (a NaN compares false: a detection that does not exist is behind everything)
                pos += (t > s || (t == s && q < d)) ? 1 : 0;
            }
            if (pos < a.max_dets) {
                rank = pos;
                s_sel[pos] = d;
            }
        }
        a.dt_rank[d0 + d] = rank;
        if (rank < 0) {
            for (int k = 0; k < nA; ++k) {
                a.dt_match[(size_t)k * a.n_dt + d0 + d] = 0u;
                a.dt_ignore[(size_t)k * a.n_dt + d0 + d] = 0u;
            }
            if (ob >= 0)
                for (int g = 0; g < G; ++g) a.oks[ob + (long long)d * G + g] = -1.0;
        }
    }
    if (mine) atomicAdd(&s_nvalid, mine);   // (an integer count: the order of the additions does not matter)
    // 2. gtIg of every area range
    for (int i = tid; i < nA * G; i += OKS_NT) {
        const int k = i / G, g = i - k * G;
        const double ar = a.gt_area[g0 + g];
        const unsigned char ig = ((s_fl[g] & 2) || ar < s_rng[2 * k] || ar > s_rng[2 * k + 1]) ? 1 : 0;
        s_ig[k][g] = ig;
        a.gt_ignore[(size_t)k * a.n_gt + g0 + g] = ig;
    }
    __syncthreads();
    const int nsel = s_nvalid < a.max_dets ? s_nvalid : a.max_dets;
    // 3. walk order: non-ignored first, stable
    for (int i = tid; i < nA * G; i += OKS_NT) {
        const int k = i / G, g = i - k * G;
        const unsigned char ig = s_ig[k][g];
        int same_before = 0, kept = 0;
        for (int q = 0; q < G; ++q) {
            const unsigned char iq = s_ig[k][q];
            kept += iq ? 0 : 1;
            same_before += (iq == ig && q < g) ? 1 : 0;
        }
        s_walk[k][ig ? kept + same_before : same_before] = (unsigned short)g;
    }
    // 4. detection areas (loadRes)
    if (tid < nsel) {
        const float* kp = a.dt_kpts + (size_t)(d0 + s_sel[tid]) * J * 2;
        float x0 = kp[0], x1 = kp[0], y0 = kp[1], y1 = kp[1];
        for (int j = 1; j < J; ++j) {
            const float x = kp[2 * j], y = kp[2 * j + 1];
            x0 = x < x0 ? x : x0;
            x1 = x > x1 ? x : x1;
            y0 = y < y0 ? y : y0;
            y1 = y > y1 ? y : y1;
        }
        s_darea[tid] = __dmul_rn((double)x1 - (double)x0, (double)y1 - (double)y0);
    }
    // 5. the OKS matrix (computeOks)
    for (int i = tid; i < nsel * G; i += OKS_NT) {
        const int r = i / G, g = i - r * G;
        const double* gk = a.gt_kpts + (size_t)(g0 + g) * J * 3;
        const float* dk = a.dt_kpts + (size_t)(d0 + s_sel[r]) * J * 2;
        int k1 = 0;
        for (int j = 0; j < J; ++j) k1 += gk[3 * j + 2] > 0.0 ? 1 : 0;
        const double den = a.gt_area[g0 + g] + OKS_EPS;
        const double* bb = a.gt_bbox + (size_t)(g0 + g) * 4;
        const double bx0 = bb[0] - bb[2], bx1 = bb[0] + bb[2] * 2.0, by0 = bb[1] - bb[3], by1 = bb[1] + bb[3] * 2.0;   // (* 2 is exact)
        double sum = 0.0;
        for (int j = 0; j < J; ++j) {
            const double xd = (double)dk[2 * j], yd = (double)dk[2 * j + 1];
            double dx, dy;
            if (k1 > 0) {
                dx = xd - gk[3 * j];
                dy = yd - gk[3 * j + 1];
            } else {
                dx = __dadd_rn(fmax(0.0, bx0 - xd), fmax(0.0, xd - bx1));
                dy = __dadd_rn(fmax(0.0, by0 - yd), fmax(0.0, yd - by1));
            }
            const double e = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) / s_var[j] / den / 2.0;
            if (k1 == 0 || gk[3 * j + 2] > 0.0) sum += exp(-e);
        }
        const double o = sum / (double)(k1 > 0 ? k1 : J);
        s_oks[i] = o;
        if (ob >= 0) a.oks[ob + (long long)s_sel[r] * G + g] = o;
    }
    __syncthreads();
    // 6. the n_area x n_thr greedy walks (evaluateImg): wave = area range, lane = threshold
    if (wave < nA) {
        const int k = wave;
        const bool act = lane < nT;
        const double lo = s_rng[2 * k], hi = s_rng[2 * k + 1];
        unsigned* gtm = s_gtm + (size_t)(k * OKS_MAX_THR + (lane & (OKS_MAX_THR - 1))) * (OKS_MAX_GT / 32);
        if (act)
            for (int w = 0; w < OKS_MAX_GT / 32; ++w) gtm[w] = 0u;
        for (int r = 0; r < nsel; ++r) {
            bool mt = false, igd = false;
            if (act) {
                double iou = fmin(s_thr[lane], 1.0 - 1e-10);
                int m = -1;
                for (int w = 0; w < G; ++w) {
                    const int g = s_walk[k][w];
                    if (((gtm[g >> 5] >> (g & 31)) & 1u) && !(s_fl[g] & 1)) continue;   // matched already, and no crowd
                    if (m > -1 && !s_ig[k][m] && s_ig[k][g]) break;                      // a real match is not traded for an ignored gt
                    const double o = s_oks[r * G + g];
                    if (o < iou) continue;
                    iou = o;
                    m = g;
                }
                if (m >= 0) {
                    mt = true;
                    igd = s_ig[k][m] != 0;
                    gtm[m >> 5] |= 1u << (m & 31);
                } else {
                    igd = s_darea[r] < lo || s_darea[r] > hi;
                }
            }
            const unsigned long long bm = __ballot(mt), bi = __ballot(igd);
            if (lane == 0) {
                const size_t at = (size_t)k * a.n_dt + d0 + s_sel[r];
                a.dt_match[at] = (unsigned)bm;
                a.dt_ignore[at] = (unsigned)bi;
            }
        }
    }
}

hipError_t oks_allow_lds() {   // (above 64 KB of LDS in all the attribute is needed; it is per device)
    static std::mutex mu;
    static bool done[64];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    if (dev < 0 || dev >= 64 || !done[dev]) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(oks_match_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)OKS_MAX_LDS);
        if (e == hipSuccess && dev >= 0 && dev < 64) done[dev] = true;
    }
    return e;
}

// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int ACC_NT = 1024;   // one chunk of the walk; 16 waves
constexpr int ACC_NW = ACC_NT / 64;

struct AccShared {
    unsigned long long v[ACC_NW];
    double m[ACC_NW];
};

// sum over the block, the same value in every thread
__device__ unsigned long long block_sum(unsigned long long v, AccShared& sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (the previous user of sh is done)
    if ((threadIdx.x & 63) == 0) sh.v[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < ACC_NW; ++w) t += sh.v[w];
    return t;
}

// inclusive prefix sum over the block in thread order; total = the block's sum
__device__ unsigned long long block_scan_sum(unsigned long long v, AccShared& sh, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    __syncthreads();
    if (lane == 63) sh.v[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < ACC_NW; ++w) {
        const unsigned long long t = sh.v[w];
        before += w < wave ? t : 0ull;
        all += t;
    }
    total = all;
    return v + before;
}

// inclusive maximum over the threads AT AND BEHIND this one; total = the block's maximum
__device__ double block_scan_max_back(double v, AccShared& sh, double& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_down(v, o);
        if (lane + o < 64) v = fmax(v, t);
    }
    __syncthreads();
    if (lane == 0) sh.m[wave] = v;
    __syncthreads();
    double behind = -1.0, all = -1.0;
    for (int w = 0; w < ACC_NW; ++w) {
        const double t = sh.m[w];
        if (w > wave) behind = fmax(behind, t);
        all = fmax(all, t);
    }
    total = all;
    return fmax(v, behind);
}

__global__ __launch_bounds__(ACC_NT) void oks_accumulate_k(const i2r_oks_accumulate_args a) {
    __shared__ AccShared sh;
    __shared__ double s_q[OKS_MAX_REC], s_rt[OKS_MAX_REC];
    const int tid = threadIdx.x;
    const int nT = a.n_thr, nA = a.n_area, R = a.n_rec;
    const int t = blockIdx.x % nT, k = (blockIdx.x / nT) % nA, grp = blockIdx.x / (nT * nA);
    const bool all = grp == a.n_group;
    const unsigned* dtm = a.dt_match + (size_t)k * a.n_dt;
    const unsigned* dti = a.dt_ignore + (size_t)k * a.n_dt;
    auto in_group = [&](int im) -> bool { return all || a.img_group[im] == grp; };
    // entry p of the walk: does it take part, and what does it count -- true positive in the high word, false positive in the low one
    auto item = [&](long long p, unsigned long long& v) -> bool {
        v = 0ull;
        if (p >= a.n_part) return false;
        const int d = a.order[p];
        if (d < 0 || d >= a.n_dt || (a.dt_rank && a.dt_rank[d] < 0)) return false;
        const int im = a.dt_img[d];
        if (im < 0 || im >= a.n_img || !in_group(im)) return false;
        if (!((dti[d] >> t) & 1u)) v = ((dtm[d] >> t) & 1u) ? 1ull << 32 : 1ull;
        return true;
    };
    // npig: the non-ignored gts of the group's images
    unsigned long long cnt = 0;
    for (int im = tid; im < a.n_img; im += ACC_NT) {
        if (!in_group(im)) continue;
        const int q0 = a.gt_off[im], q1 = a.gt_off[im + 1];
        if (q0 < 0 || q1 > a.n_gt) continue;
        for (int g = q0; g < q1; ++g) cnt += a.gt_ignore[(size_t)k * a.n_gt + g] ? 0ull : 1ull;
    }
    const unsigned long long npig = block_sum(cnt, sh);
    if (t == 0 && tid == 0) a.npig[grp * nA + k] = (int)npig;
    double* prec = a.precision + ((size_t)(grp * nT + t) * R) * nA + k;   // element r at prec[r * nA]
    double* rec = a.recall + (size_t)(grp * nT + t) * nA + k;
    if (npig == 0) {
        for (int r = tid; r < R; r += ACC_NT) prec[(size_t)r * nA] = -1.0;
        if (tid == 0) *rec = -1.0;
        return;
    }
    // pass 1: the totals
    unsigned long long sum = 0, members = 0;
    for (long long p = tid; p < a.n_part; p += ACC_NT) {
        unsigned long long v;
        members += item(p, v) ? 1ull : 0ull;
        sum += v;
    }
    const unsigned long long total = block_sum(sum, sh);
    const unsigned long long nd = block_sum(members, sh);
    for (int r = tid; r < R; r += ACC_NT) {
        s_q[r] = 0.0;
        s_rt[r] = a.rec_thr[r];
    }
    const double dn = (double)npig;
    if (tid == 0) *rec = nd ? (double)(total >> 32) / dn : 0.0;
    // pass 2: chunks from the back; `before` = the counts in front of the chunk, `carry` = the largest pr behind it
    unsigned long long before = total;
    double carry = -1.0;
    const long long nchunk = ((long long)a.n_part + ACC_NT - 1) / ACC_NT;
    for (long long c = nchunk - 1; c >= 0; --c) {
        unsigned long long v, chunk_total;
        const bool mem = item(c * ACC_NT + tid, v);
        const unsigned long long incl = block_scan_sum(v, sh, chunk_total);
        before -= chunk_total;
        const unsigned long long cum = before + incl;
        const unsigned long long tp = cum >> 32, fp = cum & 0xffffffffull;
        const double pr = mem ? (double)tp / ((double)(fp + tp) + OKS_EPS) : -1.0;   // (-1: below every pr, which are >= 0)
        double chunk_max;
        const double back = block_scan_max_back(pr, sh, chunk_max);
        const double pm = fmax(back, carry);
        carry = fmax(carry, chunk_max);
        if (mem && (v >> 32)) {   // rc rises here from (tp - 1) / npig to tp / npig: the first i of every threshold in between
            const double rc0 = (double)(tp - 1) / dn, rc1 = (double)tp / dn;
            for (int r = 0; r < R; ++r) {
                const double th = s_rt[r];
                if (th > 0.0 && th > rc0 && th <= rc1) s_q[r] = pm;   // (one writer per r)
            }
        }
    }
    __syncthreads();
    // a threshold <= 0 is met by the first entry, whose non-increasing pr is the largest of all
    for (int r = tid; r < R; r += ACC_NT) prec[(size_t)r * nA] = s_rt[r] > 0.0 ? s_q[r] : (carry >= 0.0 ? carry : 0.0);
}

}  // namespace

extern "C" int i2r_oks_match(const i2r_oks_match_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_oks_match: null args");
    I2R_CHECK_ARG(a->n_dt >= 0 && a->n_gt >= 0 && a->n_img >= 0, "i2r_oks_match: n_dt %d, n_gt %d, n_img %d", a->n_dt, a->n_gt, a->n_img);
    I2R_CHECK_ARG(a->joints >= 1 && a->joints <= 32, "i2r_oks_match: %d joints (1..32)", a->joints);
    I2R_CHECK_ARG(a->n_thr >= 1 && a->n_thr <= OKS_MAX_THR, "i2r_oks_match: %d thresholds (1..%d)", a->n_thr, OKS_MAX_THR);
    I2R_CHECK_ARG(a->n_area >= 1 && a->n_area <= OKS_MAX_AREA, "i2r_oks_match: %d area ranges (1..%d)", a->n_area, OKS_MAX_AREA);
    I2R_CHECK_ARG(a->max_dets >= 1 && a->max_dets <= OKS_MAX_DETS, "i2r_oks_match: max_dets %d over the limit (1..%d)", a->max_dets, OKS_MAX_DETS);
    I2R_CHECK_ARG(a->max_dt_per_img >= 0 && a->max_dt_per_img <= OKS_MAX_DT, "i2r_oks_match: %d detections of one image over the limit %d",
                  a->max_dt_per_img, OKS_MAX_DT);
    I2R_CHECK_ARG(a->max_gt_per_img >= 0 && a->max_gt_per_img <= OKS_MAX_GT, "i2r_oks_match: %d ground truths of one image over the limit %d",
                  a->max_gt_per_img, OKS_MAX_GT);
    if (a->n_img == 0) return I2R_OK;
    I2R_CHECK_ARG(a->dt_off && a->gt_off && a->sigmas && a->thr && a->area_rng, "i2r_oks_match: null input pointer");
    I2R_CHECK_ARG(a->n_dt == 0 || (a->dt_kpts && a->dt_score && a->dt_rank && a->dt_match && a->dt_ignore), "i2r_oks_match: null detection pointer");
    I2R_CHECK_ARG(a->n_gt == 0 || (a->gt_kpts && a->gt_area && a->gt_bbox && a->gt_flags && a->gt_ignore), "i2r_oks_match: null ground-truth pointer");
    I2R_CHECK_ARG(!a->oks || (a->oks_off && a->oks_len >= 0), "i2r_oks_match: oks without oks_off / oks_len");
    const int md = a->max_dets < a->max_dt_per_img ? a->max_dets : a->max_dt_per_img;
    size_t lds = (size_t)md * (size_t)a->max_gt_per_img * 8;
    if (lds < 8) lds = 8;
    if (lds > 48 * 1024) {
        const hipError_t e = oks_allow_lds();
        if (e != hipSuccess) {
            i2r_set_error("i2r_oks_match: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
            return I2R_E_LAUNCH;
        }
    }
    i2r_launch(oks_match_k, dim3((unsigned)a->n_img), dim3(OKS_NT), lds, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_oks_match");
    return I2R_OK;
}

extern "C" int i2r_oks_accumulate(const i2r_oks_accumulate_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_oks_accumulate: null args");
    I2R_CHECK_ARG(a->n_dt >= 0 && a->n_gt >= 0 && a->n_img >= 0 && a->n_part >= 0 && a->n_group >= 0,
                  "i2r_oks_accumulate: n_dt %d, n_gt %d, n_img %d, n_part %d, n_group %d", a->n_dt, a->n_gt, a->n_img, a->n_part, a->n_group);
    I2R_CHECK_ARG(a->n_thr >= 1 && a->n_thr <= OKS_MAX_THR, "i2r_oks_accumulate: %d thresholds (1..%d)", a->n_thr, OKS_MAX_THR);
    I2R_CHECK_ARG(a->n_area >= 1 && a->n_area <= OKS_MAX_AREA, "i2r_oks_accumulate: %d area ranges (1..%d)", a->n_area, OKS_MAX_AREA);
    I2R_CHECK_ARG(a->n_rec >= 1 && a->n_rec <= OKS_MAX_REC, "i2r_oks_accumulate: %d recall thresholds (1..%d)", a->n_rec, OKS_MAX_REC);
    I2R_CHECK_ARG((long long)(a->n_group + 1) * a->n_thr * a->n_area <= 0x7fffffffll, "i2r_oks_accumulate: %d groups", a->n_group);
    I2R_CHECK_ARG(a->rec_thr && a->precision && a->recall && a->npig, "i2r_oks_accumulate: null rec_thr / output pointer");
    I2R_CHECK_ARG(a->n_img == 0 || a->gt_off, "i2r_oks_accumulate: null gt_off");
    I2R_CHECK_ARG(a->n_gt == 0 || a->gt_ignore, "i2r_oks_accumulate: null gt_ignore");
    I2R_CHECK_ARG(a->n_group == 0 || a->n_img == 0 || a->img_group, "i2r_oks_accumulate: null img_group with %d groups", a->n_group);
    I2R_CHECK_ARG(a->n_part == 0 || (a->order && a->dt_img && a->dt_match && a->dt_ignore), "i2r_oks_accumulate: null detection pointer");
    i2r_launch(oks_accumulate_k, dim3((unsigned)((a->n_group + 1) * a->n_thr * a->n_area)), dim3(ACC_NT), 0, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_oks_accumulate");
    return I2R_OK;
}
