// The two numbers validate() logs per batch (lib/core/function.py:167-172), on device:
//   i2r_joint_targets   JointsDataset.generate_target + adjust_target_weight (lib/dataset/JointsDataset.py:394-450)
//   i2r_val_metrics     JointsMSELoss.forward (lib/core/loss.py:15-41) + accuracy (lib/core/evaluate.py:16-71) in ONE pass over the prediction
//   i2r_val_combine     the finishing step of i2r_val_metrics over the raw sums of several parts (the shards of a data-parallel step)
// One workgroup per (crop, joint) map: the map is read once and yields the squared-error sum (fp32 terms as torch rounds them, added up
// in fp64), the first-index arg-max of the prediction and that of the target.  In analytic mode the target value of a pixel is evaluated
// from (mu_x, mu_y, weight) and never stored or read.  A second launch of one workgroup adds the per-map partials up in a fixed order (no
// floating-point atomics: two runs give the same bits) and applies calc_dists / dist_acc / the two AverageMeter updates.
// Latency kernels: config 3's batch is 798 maps of 12 KB, a few microseconds of HBM time.
#include "i2r_common.h"
#include "i2r_targets.h"  // joint_weight, gauss: the target of a (crop, joint) map, shared with i2r_head_fit.hip

// Every product and difference below is a rounding of its own (torch's four fp32 operations per loss term, numpy's float64 steps of the
// Gaussian's argument and of calc_dists).  HIP device code contracts a * b - c to an FMA by default.  __fmul_rn / __fsub_rn do not stop
// that here: the headers define them as plain `x * y` / `x - y` compiled with contraction allowed, and once inlined the pair was fused
// (seen in the ISA of the 16-byte path, and as a 7e-9 relative error of the weighted sums).  So contraction is switched off for this
// file and the arithmetic is written with plain operators, which the pragma governs.
#pragma clang fp contract(off)

namespace {

constexpr int MET_NT = 256;   // 4 waves per map
constexpr int FIN_NT = 1024;  // 16 waves: wave k finishes joints k, k + 16, ...
constexpr int CMB_NT = 256;   // i2r_val_combine: thread k totals joints k, k + 256, ...

// np.argmax order: a NaN beats every number, then the larger value, then the lower flat index
__device__ inline bool beats(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn) return i < bi;
    return v > bv || (v == bv && i < bi);
}

struct Part {
    double sse;
    float pv, tv;
    int pi, ti;
};

__device__ inline void part_add(Part& a, float p, float t, int i, float wt, bool use_w) {
    const float d = use_w ? p * wt - t * wt : p - t;
    a.sse += (double)(d * d);
    if (beats(p, i, a.pv, a.pi)) { a.pv = p; a.pi = i; }
    if (beats(t, i, a.tv, a.ti)) { a.tv = t; a.ti = i; }
}

__device__ inline void part_merge(Part& a, double sse, float pv, int pi, float tv, int ti) {
    a.sse += sse;
    if (beats(pv, pi, a.pv, a.pi)) { a.pv = pv; a.pi = pi; }
    if (beats(tv, ti, a.tv, a.ti)) { a.tv = tv; a.ti = ti; }
}

// workspace of i2r_val_metrics: per map one double (sum of squared errors) and two int32 (arg-max of prediction / target, -1 = max <= 0)
__host__ __device__ inline double* ws_sse(void* ws) { return reinterpret_cast<double*>(ws); }
__host__ __device__ inline int* ws_idx(void* ws, size_t n_maps) { return reinterpret_cast<int*>(ws_sse(ws) + n_maps); }

template <bool ANALYTIC>
__global__ __launch_bounds__(MET_NT) void val_metrics_map_k(const i2r_val_metrics_args a) {
    __shared__ double r_sse[MET_NT / 64];
    __shared__ float r_pv[MET_NT / 64], r_tv[MET_NT / 64];
    __shared__ int r_pi[MET_NT / 64], r_ti[MET_NT / 64];
    const size_t map = blockIdx.x, n_maps = (size_t)a.n_crops * a.joints;
    const int j = (int)(map % a.joints), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = a.h * a.w, w = a.w;
    const float* p = a.output + map * hw;
    const float* t = ANALYTIC ? nullptr : a.target + map * hw;
    const bool use_w = a.use_target_weight != 0;
    float wt = 1.f;
    bool draw = false;
    double mx = 0.0, my = 0.0;
    const double two_s2 = 2.0 * a.sigma * a.sigma;
    if (ANALYTIC) {
        mx = a.joints_hm[map * 2];
        my = a.joints_hm[map * 2 + 1];
        wt = joint_weight(mx, my, a.joints_vis[map], a.joints_weight, j, a.sigma, a.h, a.w, &draw);
    } else if (use_w) {
        wt = a.target_weight[map];
    }
    Part acc = {0.0, -__builtin_inff(), -__builtin_inff(), 0x7fffffff, 0x7fffffff};
    // 16-byte loads where every map starts on a 16-byte boundary; otherwise (h * w not a multiple of 4, or an offset base) scalar ones
    const bool wide = (hw & 3) == 0 && ((uintptr_t)a.output & 15) == 0 && (ANALYTIC || ((uintptr_t)a.target & 15) == 0);
    if (wide) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4* t4 = reinterpret_cast<const float4*>(t);
        for (int q = tid; q < (hw >> 2); q += MET_NT) {
            const float4 pv = p4[q];
            float tv[4];
            if (ANALYTIC) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = q * 4 + k;
                    tv[k] = draw ? gauss(i % w, i / w, mx, my, two_s2) : 0.f;
                }
            } else {
                const float4 v = t4[q];
                tv[0] = v.x; tv[1] = v.y; tv[2] = v.z; tv[3] = v.w;
            }
            part_add(acc, pv.x, tv[0], q * 4, wt, use_w);
            part_add(acc, pv.y, tv[1], q * 4 + 1, wt, use_w);
            part_add(acc, pv.z, tv[2], q * 4 + 2, wt, use_w);
            part_add(acc, pv.w, tv[3], q * 4 + 3, wt, use_w);
        }
    } else {
        for (int i = tid; i < hw; i += MET_NT) {
            const float tv = ANALYTIC ? (draw ? gauss(i % w, i / w, mx, my, two_s2) : 0.f) : t[i];
            part_add(acc, p[i], tv, i, wt, use_w);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        part_merge(acc, __shfl_xor(acc.sse, o), __shfl_xor(acc.pv, o), __shfl_xor(acc.pi, o), __shfl_xor(acc.tv, o), __shfl_xor(acc.ti, o));
    if (lane == 0) { r_sse[wave] = acc.sse; r_pv[wave] = acc.pv; r_pi[wave] = acc.pi; r_tv[wave] = acc.tv; r_ti[wave] = acc.ti; }
    __syncthreads();
    if (tid == 0) {
        Part all = {r_sse[0], r_pv[0], r_tv[0], r_pi[0], r_ti[0]};
        for (int k = 1; k < MET_NT / 64; ++k) part_merge(all, r_sse[k], r_pv[k], r_pi[k], r_tv[k], r_ti[k]);
        // get_max_preds (inference.py:39-47): (idx % w, floor(idx / w)), both zeroed unless max > 0 (a NaN maximum is not > 0)
        const bool p_on = all.pv > 0.f, t_on = all.tv > 0.f;
        a.pred[map * 2] = p_on ? (float)(all.pi % w) : 0.f;
        a.pred[map * 2 + 1] = p_on ? (float)(all.pi / w) : 0.f;
        ws_sse(a.ws)[map] = all.sse;
        int* idx = ws_idx(a.ws, n_maps);
        idx[map * 2] = p_on ? all.pi : -1;
        idx[map * 2 + 1] = t_on ? all.ti : -1;
    }
}

// accuracy() behind get_max_preds (evaluate.py:41-71) and the loss's means, one workgroup, every sum in a fixed order
__global__ __launch_bounds__(FIN_NT) void val_metrics_finish_k(const i2r_val_metrics_args a) {
    const int S = a.n_crops, J = a.joints, w = a.w, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n_maps = (size_t)S * J;
    const double* m_sse = ws_sse(a.ws);
    const int* m_idx = ws_idx(a.ws, n_maps);
    const double n0 = (double)a.h / 10.0, n1 = (double)a.w / 10.0;  // norm = [h, w] / 10 meets (x, y) in that order: x / (h / 10)
    for (int j = wave; j < J; j += FIN_NT / 64) {
        double sse = 0.0;
        int hits = 0, valid = 0;
        for (int s = lane; s < S; s += 64) {
            const size_t map = (size_t)s * J + j;
            sse += m_sse[map];
            const int pi = m_idx[map * 2], ti = m_idx[map * 2 + 1];
            const double px = pi < 0 ? 0.0 : (double)(pi % w), py = pi < 0 ? 0.0 : (double)(pi / w);
            const double tx = ti < 0 ? 0.0 : (double)(ti % w), ty = ti < 0 ? 0.0 : (double)(ti / w);
            if (tx > 1.0 && ty > 1.0) {  // calc_dists: only a target arg-max with x > 1 and y > 1 counts
                const double dx = px / n0 - tx / n0, dy = py / n1 - ty / n1;
                const double dist = sqrt(dx * dx + dy * dy);
                ++valid;
                hits += dist < 0.5 ? 1 : 0;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sse += __shfl_xor(sse, o);
            hits += __shfl_xor(hits, o);
            valid += __shfl_xor(valid, o);
        }
        if (lane == 0) {
            a.sse[j] = sse;
            a.hits[j] = hits;
            a.valid[j] = valid;
            a.acc[j + 1] = valid > 0 ? (double)hits * 1.0 / (double)valid : -1.0;  // dist_acc
        }
    }
    __syncthreads();  // (the values above were written by this workgroup: visible to it behind the barrier)
    if (tid == 0) {
        const double n_px = (double)S * (double)a.h * (double)a.w;
        double loss = 0.0, avg = 0.0;
        int cnt = 0;
        for (int j = 0; j < J; ++j) {
            loss += 0.5 * (a.sse[j] / n_px);
            const double v = a.acc[j + 1];
            if (v >= 0.0) { avg += v; ++cnt; }
        }
        loss /= (double)J;
        avg = cnt != 0 ? avg / (double)cnt : 0.0;
        *a.loss = loss;
        *a.avg_acc = avg;
        *a.cnt = cnt;
        a.acc[0] = avg;  // (0 when cnt == 0, as np.zeros leaves it)
        if (a.meter) {   // AverageMeter.update(loss, S) and .update(avg_acc, cnt), function.py:168-174: sum += val * n, count += n
            a.meter[0] += loss * (double)S;
            a.meter[1] += (double)S;
            a.meter[2] += avg * (double)cnt;
            a.meter[3] += (double)cnt;
        }
    }
}

// The tail of val_metrics_finish_k over the totals of n_part rows (n_crops, sse[J], hits[J], valid[J]) of doubles.  A thread owns whole
// joints and walks the parts in ascending order: no cross-lane sum, so the order of every addition is the part index and nothing else.
// The counts are integers held in doubles, exact below 2^53; their totals fit an int by the entry's precondition.
__global__ __launch_bounds__(CMB_NT) void val_combine_k(const i2r_val_combine_args a) {
    const int J = a.joints, P = a.n_part, tid = threadIdx.x;
    const size_t row = 1 + 3 * (size_t)J;
    double crops = 0.0;  // (every thread adds the same integers in the same order: the same total)
    for (int r = 0; r < P; ++r) {
        const double n = a.parts[r * row];
        if (n > 0.0) crops += n;
    }
    const bool any = crops > 0.0;
    for (int j = tid; j < J; j += CMB_NT) {
        double sse = 0.0, hits = 0.0, valid = 0.0;
        for (int r = 0; r < P; ++r) {
            const double* p = a.parts + r * row;
            if (!(p[0] > 0.0)) continue;  // a rank without crops (or a NaN count) contributes nothing
            sse += p[1 + j];
            hits += p[1 + J + j];
            valid += p[1 + 2 * (size_t)J + j];
        }
        const int h_i = (int)hits, v_i = (int)valid;
        a.sse[j] = sse;
        a.hits[j] = h_i;
        a.valid[j] = v_i;
        a.acc[j + 1] = !any ? 0.0 : v_i > 0 ? (double)h_i * 1.0 / (double)v_i : -1.0;  // dist_acc
    }
    __syncthreads();  // (the values above were written by this workgroup: visible to it behind the barrier)
    if (tid == 0) {
        const int S = (int)crops;
        *a.n_crops = S;
        if (!any) {  // no crop anywhere: zeros, the meter left alone, nothing divided
            *a.loss = 0.0;
            *a.avg_acc = 0.0;
            *a.cnt = 0;
            a.acc[0] = 0.0;
            return;
        }
        const double n_px = (double)S * (double)a.h * (double)a.w;
        double loss = 0.0, avg = 0.0;
        int cnt = 0;
        for (int j = 0; j < J; ++j) {
            loss += 0.5 * (a.sse[j] / n_px);
            const double v = a.acc[j + 1];
            if (v >= 0.0) { avg += v; ++cnt; }
        }
        loss /= (double)J;
        avg = cnt != 0 ? avg / (double)cnt : 0.0;
        *a.loss = loss;
        *a.avg_acc = avg;
        *a.cnt = cnt;
        a.acc[0] = avg;
        if (a.meter) {
            a.meter[0] += loss * (double)S;
            a.meter[1] += (double)S;
            a.meter[2] += avg * (double)cnt;
            a.meter[3] += (double)cnt;
        }
    }
}

__global__ __launch_bounds__(MET_NT) void joint_targets_k(const i2r_joint_targets_args a) {
    const size_t map = blockIdx.x;
    const int j = (int)(map % a.joints), hw = a.h * a.w, w = a.w;
    const double mx = a.joints_hm[map * 2], my = a.joints_hm[map * 2 + 1];
    bool draw;
    const float wt = joint_weight(mx, my, a.joints_vis[map], a.joints_weight, j, a.sigma, a.h, a.w, &draw);
    if (threadIdx.x == 0) a.target_weight[map] = wt;
    if (!a.target) return;
    const double two_s2 = 2.0 * a.sigma * a.sigma;
    float* t = a.target + map * hw;
    for (int i = threadIdx.x; i < hw; i += MET_NT) t[i] = draw ? gauss(i % w, i / w, mx, my, two_s2) : 0.f;
}

// the launch grid is one workgroup per map: the count must fit the grid's x dimension
bool maps_fit(int s, int j, int h, int w) {
    return (long long)s * j <= 0x7fffffffLL && (long long)h * w <= 0x7fffffffLL;
}

}  // namespace

extern "C" int i2r_joint_targets(const i2r_joint_targets_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_joint_targets: null args");
    I2R_CHECK_ARG(a->n_crops >= 0 && a->joints >= 1 && a->h >= 1 && a->w >= 1, "i2r_joint_targets: %d crops, %d joints, %d x %d", a->n_crops,
                  a->joints, a->h, a->w);
    I2R_CHECK_ARG(maps_fit(a->n_crops, a->joints, a->h, a->w), "i2r_joint_targets: %d x %d maps of %d x %d", a->n_crops, a->joints, a->h, a->w);
    I2R_CHECK_ARG(a->sigma > 0.0, "i2r_joint_targets: sigma %g", a->sigma);
    if (a->n_crops == 0) return I2R_OK;
    I2R_CHECK_ARG(a->joints_hm && a->joints_vis && a->target_weight, "i2r_joint_targets: null joints_hm / joints_vis / target_weight");
    i2r_launch(joint_targets_k, dim3((unsigned)(a->n_crops * a->joints)), dim3(MET_NT), 0, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_joint_targets");
    return I2R_OK;
}

extern "C" int i2r_val_metrics(const i2r_val_metrics_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_val_metrics: null args");
    I2R_CHECK_ARG(a->n_crops >= 0 && a->joints >= 1 && a->h >= 1 && a->w >= 1, "i2r_val_metrics: %d crops, %d joints, %d x %d", a->n_crops,
                  a->joints, a->h, a->w);
    I2R_CHECK_ARG(maps_fit(a->n_crops, a->joints, a->h, a->w), "i2r_val_metrics: %d x %d maps of %d x %d", a->n_crops, a->joints, a->h, a->w);
    const bool tensor = a->target != nullptr, analytic = a->joints_hm != nullptr;
    I2R_CHECK_ARG(tensor != analytic, "i2r_val_metrics: %s target form given (target tensor, or joints_hm + joints_vis)", tensor ? "more than one" : "no");
    I2R_CHECK_ARG(!analytic || (a->target_weight == nullptr && a->joints_vis != nullptr),
                  "i2r_val_metrics: the analytic form takes joints_vis and no target_weight");
    I2R_CHECK_ARG(!analytic || a->sigma > 0.0, "i2r_val_metrics: sigma %g", a->sigma);
    I2R_CHECK_ARG(!tensor || a->target_weight || !a->use_target_weight, "i2r_val_metrics: use_target_weight without target_weight");
    if (a->n_crops == 0) return I2R_OK;
    I2R_CHECK_ARG(a->output && a->ws, "i2r_val_metrics: null output / workspace");
    I2R_CHECK_ARG(((uintptr_t)a->ws & 7) == 0, "i2r_val_metrics: workspace not 8-byte aligned");
    I2R_CHECK_ARG(a->loss && a->acc && a->avg_acc && a->cnt && a->pred && a->sse && a->hits && a->valid, "i2r_val_metrics: null result pointer");
    const dim3 grid((unsigned)(a->n_crops * a->joints));
    if (analytic)
        i2r_launch(val_metrics_map_k<true>, grid, dim3(MET_NT), 0, (hipStream_t)stream, *a);
    else
        i2r_launch(val_metrics_map_k<false>, grid, dim3(MET_NT), 0, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_val_metrics");
    i2r_launch(val_metrics_finish_k, dim3(1), dim3(FIN_NT), 0, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_val_metrics (finish)");
    return I2R_OK;
}

extern "C" int i2r_val_combine(const i2r_val_combine_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_val_combine: null args");
    I2R_CHECK_ARG(a->n_part >= 1 && a->joints >= 1 && a->h >= 1 && a->w >= 1, "i2r_val_combine: %d parts, %d joints, %d x %d", a->n_part,
                  a->joints, a->h, a->w);
    I2R_CHECK_ARG(a->parts, "i2r_val_combine: null parts");
    I2R_CHECK_ARG(a->sse && a->hits && a->valid && a->loss && a->acc && a->avg_acc && a->cnt && a->n_crops, "i2r_val_combine: null result pointer");
    i2r_launch(val_combine_k, dim3(1), dim3(CMB_NT), 0, (hipStream_t)stream, *a);
    I2R_CHECK_LAUNCH("i2r_val_combine");
    return I2R_OK;
}
