// Head re-fit: the gradient of JointsMSELoss (lib/core/loss.py:15-41) with respect to final_layer (a 1x1 conv with bias) on frozen
// features, in one pass over the features:
//   i2r_head_grad   o = W f + b per pixel, g = tw^2 (o - t), dW = sum g f^T / (N J), db = sum g / (N J), sse and the loss
// The heat map o, the target t and the gradient map g exist only in registers.  Two launches:
//   tile    one wave per workgroup owns a run of 16-pixel fragments of ONE crop.  Per fragment the feature rows are loaded once (16-byte
//           loads along the channels), O = F W^T runs on the fp32 matrix pipe with the k-permutation of i2r_head, and its D layout -- lane
//           (joint n, g) holds pixels 4 g .. 4 g + 3 -- is already the A operand of dW += G^T F with k = the pixel: G never leaves the
//           registers, and the target is read (16 bytes of a joint's NCHW plane per lane) or evaluated in that layout.  Only F takes the
//           way through LDS, to be read back as the B operand (lane (channel c, g) wants pixel 4 g + r, channel 16 cb + c).
//           The wave writes its partial dW (fp32: at most one crop's pixels), db and sse (fp64) to the workspace.
//   finish  adds the partials up in fp64 in a fixed order (64 or 32 interleaved slices per output, each in ascending part index, then the
//           slices in ascending order), divides once by N J in fp64 and rounds once to fp32.
// No floating-point atomics: two runs give the same bits.  The split into parts depends on the shape alone.
#include "i2r_common.h"
#include "i2r_targets.h"  // joint_weight, gauss (contraction is off from here on: the loss terms are torch's four fp32 operations)

namespace {

constexpr int HG_LS = 128 + 4;    // floats per pixel row of the LDS feature image (+ 4: the four pixel groups of a B read hit disjoint banks)
constexpr int HG_WAVES = 2048;    // parts aimed at: two waves per SIMD of the chip (each hides the other's load latency)
constexpr int FIN_NT = 1024;
constexpr int FIN_UNROLL = 8;     // partials a finish thread has in flight
constexpr int FIN_COLS = 16, FIN_SLICES = FIN_NT / FIN_COLS;   // finish, dW / db: 16 outputs x 64 slices per workgroup
constexpr int FIN_JP = 32, FIN_JSLICES = FIN_NT / FIN_JP;      // finish, sse: 32 joints x 32 slices in the last workgroup

// How the pixels are split into parts (a function of the shape alone: i2r_head_grad_ws_bytes and the launch agree by construction)
struct Plan {
    int frags_per_crop, frags_per_wave, waves_per_crop;
    long long n_part;
};

__host__ __device__ inline Plan make_plan(int n_crops, int hw) {
    Plan p;
    p.frags_per_crop = (hw + 15) / 16;
    const long long total = (long long)n_crops * p.frags_per_crop;
    long long fpw = (total + HG_WAVES - 1) / HG_WAVES;
    if (fpw < 1) fpw = 1;
    if (fpw > p.frags_per_crop) fpw = p.frags_per_crop;
    p.frags_per_wave = (int)fpw;
    p.waves_per_crop = (p.frags_per_crop + p.frags_per_wave - 1) / p.frags_per_wave;
    p.n_part = (long long)n_crops * p.waves_per_crop;
    return p;
}

// workspace: sse double [n_part][J], db double [n_part][J], dW float [n_part][J][cin]
__host__ __device__ inline double* ws_sse(void* ws) { return reinterpret_cast<double*>(ws); }
__host__ __device__ inline double* ws_db(void* ws, size_t n_part, int J) { return ws_sse(ws) + n_part * J; }
__host__ __device__ inline float* ws_dw(void* ws, size_t n_part, int J) { return reinterpret_cast<float*>(ws_db(ws, n_part, J) + n_part * J); }

// NF: 16-joint fragments (1 or 2); CJ: 16-channel steps compiled in (2, 4, 6 or 8 -- the smallest that holds cin; the steps behind
// cin run on zero rows of F and W, which add +0 to every chain)
template <int NF, int CJ, bool ANALYTIC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void head_grad_tile_k(const i2r_head_grad_args a, const Plan plan) {
    __shared__ __attribute__((aligned(16))) float fl[16 * HG_LS];
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    const size_t part = blockIdx.x, n_part = (size_t)plan.n_part;
    const int crop = (int)(part / plan.waves_per_crop), wi = (int)(part % plan.waves_per_crop);
    const int J = a.joints, cin = a.cin, cj = cin >> 4, hw = a.h * a.w_, wd = a.w_;
    const bool use_w = a.use_target_weight != 0;
    const int f0 = wi * plan.frags_per_wave, f1 = min(f0 + plan.frags_per_wave, plan.frags_per_crop);

    // W as the B operand of O = F W^T: lane (joint n, g) holds w[n][16 j + 4 g + s]; zero rows for the padding joints
    f32x4 wb[NF][CJ];
    float bj[NF], tw[NF], tw2[NF];
    bool draw[NF], on[NF];
    double mx[NF], my[NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int jn = nf * 16 + n;
        on[nf] = jn < J;
        bj[nf] = on[nf] ? a.bias[jn] : 0.f;
#pragma unroll
        for (int j = 0; j < CJ; ++j) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (on[nf] && j < cj) {
                const float* wr = a.w + (size_t)jn * a.w_cs + j * 16 + g * 4;
                v = (f32x4){wr[0], wr[1], wr[2], wr[3]};
            }
            wb[nf][j] = v;
        }
        tw[nf] = 1.f;
        draw[nf] = false;
        mx[nf] = my[nf] = 0.0;
        if (on[nf]) {
            const size_t map = (size_t)crop * J + jn;
            if (ANALYTIC) {
                mx[nf] = a.joints_hm[map * 2];
                my[nf] = a.joints_hm[map * 2 + 1];
                tw[nf] = joint_weight(mx[nf], my[nf], a.joints_vis[map], a.joints_weight, jn, a.sigma, a.h, a.w_, &draw[nf]);
            } else if (use_w) {
                tw[nf] = a.target_weight[map];
            }
        }
        tw2[nf] = use_w ? tw[nf] * tw[nf] : 1.f;
    }
    const double two_s2 = 2.0 * a.sigma * a.sigma;
    const bool vec = !ANALYTIC && (hw & 3) == 0 && ((uintptr_t)a.target & 15) == 0;  // a lane's four target pixels: one 16-byte load

    f32x4 dw[NF][CJ];
    double sse[NF], db[NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        sse[nf] = db[nf] = 0.0;
#pragma unroll
        for (int j = 0; j < CJ; ++j) dw[nf][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    const float* fcrop = a.feat + (size_t)crop * hw * a.in_cs;
    f32x4 va[CJ];
    auto load_rows = [&](int f) {  // lane (pixel m = n, g): in[pixel][16 j + 4 g .. + 3]; zero rows behind the crop's last pixel
        const int p = f * 16 + n;
        const bool ok = f < f1 && p < hw;
        const f32x4* x = reinterpret_cast<const f32x4*>(fcrop + (size_t)(ok ? p : 0) * a.in_cs) + g;
#pragma unroll
        for (int j = 0; j < CJ; ++j) va[j] = (ok && j < cj) ? x[j * 4] : (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    // the target of the lane's (joint, four pixels from pd = 16 f + 4 g) of fragment f: read (or evaluated) one fragment ahead as well
    float tn[NF][4];
    auto load_target = [&](int f) {
        const int pd = f * 16 + 4 * g;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) tn[nf][r] = 0.f;
            if (f >= f1 || !on[nf] || pd >= hw) continue;
            if (ANALYTIC) {
                if (draw[nf]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (pd + r < hw) tn[nf][r] = gauss((pd + r) % wd, (pd + r) / wd, mx[nf], my[nf], two_s2);
                }
            } else {
                const float* t = a.target + ((size_t)crop * J + nf * 16 + n) * hw + pd;
                if (vec) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(t);
                    tn[nf][0] = v[0]; tn[nf][1] = v[1]; tn[nf][2] = v[2]; tn[nf][3] = v[3];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (pd + r < hw) tn[nf][r] = t[r];
                }
            }
        }
    };
    load_rows(f0);
    load_target(f0);
#pragma nounroll
    for (int f = f0; f < f1; ++f) {
        const int pd = f * 16 + 4 * g;  // this lane's first pixel of O and G
        float tv[NF][4];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r) tv[nf][r] = tn[nf][r];
#pragma unroll
        for (int j = 0; j < CJ; ++j)
            *reinterpret_cast<f32x4*>(&fl[n * HG_LS + j * 16 + g * 4]) = va[j];
        // O = F W^T + b: D of lane (joint n, g), register r = pixel pd + r
        f32x4 o[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) o[nf] = (f32x4){bj[nf], bj[nf], bj[nf], bj[nf]};
#pragma unroll
        for (int j = 0; j < CJ; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) o[nf] = mfma16(va[j][s], wb[nf][j][s], o[nf]);
        load_rows(f + 1);  // (in flight behind the second product)
        load_target(f + 1);
        // G, and the sums that need no feature
        f32x4 gv[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float gg = 0.f;
                if (on[nf] && pd + r < hw) {
                    const float p = o[nf][r], t = tv[nf][r];
                    const float d = use_w ? p * tw[nf] - t * tw[nf] : p - t;  // the loss term as i2r_val_metrics forms it
                    sse[nf] += (double)(d * d);
                    gg = tw2[nf] * (p - t);
                    db[nf] += (double)gg;
                }
                gv[nf][r] = gg;
            }
        }
        __syncthreads();  // the feature rows are in LDS
        // dW += G^T F: A = G (lane (joint n, k = g): pixel 4 g + r), B = F (lane (channel c = n, k = g): the same pixel)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cb = 0; cb < CJ; ++cb) {
                const float b = fl[(4 * g + r) * HG_LS + cb * 16 + n];
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) dw[nf][cb] = mfma16(gv[nf][r], b, dw[nf][cb]);
            }
        __syncthreads();  // ... and read, before the next fragment overwrites them
    }

    // D of dW: lane (channel c = n, g), register r = joint 16 nf + 4 g + r
    float* pw = ws_dw(a.ws, n_part, J) + part * (size_t)J * cin;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
        for (int cb = 0; cb < CJ; ++cb)
            if (cb < cj) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jq = nf * 16 + 4 * g + r;
                    if (jq < J) pw[(size_t)jq * cin + cb * 16 + n] = dw[nf][cb][r];
                }
            }
    // sse, db of joint n: the four pixel groups in ascending order
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        double s = __shfl(sse[nf], n), d = __shfl(db[nf], n);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            s += __shfl(sse[nf], n + 16 * k);
            d += __shfl(db[nf], n + 16 * k);
        }
        if (g == 0 && on[nf]) {
            ws_sse(a.ws)[part * J + nf * 16 + n] = s;
            ws_db(a.ws, n_part, J)[part * J + nf * 16 + n] = d;
        }
    }
}

// slice k of an output: p[q * stride] for q = k, k + slices, ... added in ascending order; FIN_UNROLL loads are in flight at a time (a
// part behind the last one counts as +0.0, which changes no sum)
template <typename T>
__device__ inline double slice_sum(const T* p, size_t stride, int k, int slices, size_t n_part) {
    double s = 0.0;
    for (size_t q = k; q < n_part; q += (size_t)slices * FIN_UNROLL) {
        double v[FIN_UNROLL];
#pragma unroll
        for (int u = 0; u < FIN_UNROLL; ++u) {
            const size_t i = q + (size_t)u * slices;
            v[u] = i < n_part ? (double)p[i * stride] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < FIN_UNROLL; ++u) s += v[u];
    }
    return s;
}

// Every output is the fp64 sum of its n_part partials: slice k adds parts k, k + K, ... in ascending order, then the slices are added in
// ascending order by one thread.  Workgroups [0, n_colblk): 16 columns of (dW | db) each; the last workgroup: sse and the loss.
__global__ __launch_bounds__(FIN_NT) void head_grad_finish_k(const i2r_head_grad_args a, const Plan plan, int n_colblk) {
    __shared__ double red[FIN_SLICES][FIN_COLS + 1];
    __shared__ double jred[FIN_JSLICES][FIN_JP + 1];
    __shared__ double jtot[FIN_JP];
    const int J = a.joints, cin = a.cin, tid = threadIdx.x;
    const size_t n_part = (size_t)plan.n_part;
    const double n_px = (double)a.n_crops * (double)a.h * (double)a.w_;
    if ((int)blockIdx.x < n_colblk) {
        const int e = tid % FIN_COLS, k = tid / FIN_COLS, JC = J * cin;
        const int col = blockIdx.x * FIN_COLS + e;
        double s = 0.0;
        if (col < JC) {
            const float* p = ws_dw(a.ws, n_part, J) + col;
            s = slice_sum(p, (size_t)JC, k, FIN_SLICES, n_part);
        } else if (col < JC + J) {
            const double* p = ws_db(a.ws, n_part, J) + (col - JC);
            s = slice_sum(p, (size_t)J, k, FIN_SLICES, n_part);
        }
        red[k][e] = s;
        __syncthreads();
        if (k == 0 && col < JC + J) {
            double tot = 0.0;
            for (int kk = 0; kk < FIN_SLICES; ++kk) tot += red[kk][e];
            const float v = (float)(tot / (n_px * (double)J));
            if (col < JC) a.dw[col] = v; else a.db[col - JC] = v;
        }
        return;
    }
    const int j = tid % FIN_JP, k = tid / FIN_JP;
    double s = 0.0;
    if (j < J) {
        const double* p = ws_sse(a.ws) + j;
        s = slice_sum(p, (size_t)J, k, FIN_JSLICES, n_part);
    }
    jred[k][j] = s;
    __syncthreads();
    if (tid < FIN_JP) {
        double tot = 0.0;
        for (int kk = 0; kk < FIN_JSLICES; ++kk) tot += jred[kk][tid];
        jtot[tid] = tot;
        if (tid < J) a.sse[tid] = tot;
    }
    __syncthreads();
    if (tid == 0) {  // the loss's means as i2r_val_metrics takes them
        double loss = 0.0;
        for (int jj = 0; jj < J; ++jj) loss += 0.5 * (jtot[jj] / n_px);
        *a.loss = loss / (double)J;
    }
}

bool shape_ok(int n_crops, int h, int w, int cin, int joints) {
    return n_crops >= 0 && h >= 1 && w >= 1 && joints >= 1 && joints <= 32 && cin >= 16 && cin <= 128 && cin % 16 == 0 &&
           (long long)h * w <= 0x7fffffffLL - 64 && (long long)n_crops * (((long long)h * w + 15) / 16) <= 0x7fffffffLL &&
           (long long)n_crops * joints <= 0x7fffffffLL;
}

}  // namespace

extern "C" int i2r_head_grad_ws_bytes(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t* bytes) {
    I2R_CHECK_ARG(bytes, "i2r_head_grad_ws_bytes: null result pointer");
    I2R_CHECK_ARG(shape_ok(n_crops, h, w_, cin, joints), "i2r_head_grad_ws_bytes: %d crops, %d x %d, cin=%d, joints=%d", n_crops, h, w_, cin, joints);
    const Plan p = make_plan(n_crops, h * w_);
    *bytes = p.n_part * ((int64_t)joints * 16 + (int64_t)joints * cin * 4);
    return I2R_OK;
}

extern "C" int i2r_head_grad(const i2r_head_grad_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_head_grad: null args");
    I2R_CHECK_ARG(shape_ok(a->n_crops, a->h, a->w_, a->cin, a->joints), "i2r_head_grad: %d crops, %d x %d, cin=%d (a multiple of 16 in [16, 128]), joints=%d (1 .. 32)",
                  a->n_crops, a->h, a->w_, a->cin, a->joints);
    I2R_CHECK_ARG(a->cin <= a->in_cs && a->cin <= a->w_cs && a->in_cs % 4 == 0, "i2r_head_grad: cin=%d in_cs=%d w_cs=%d", a->cin, a->in_cs, a->w_cs);
    I2R_CHECK_ARG(((uintptr_t)a->feat & 15) == 0, "i2r_head_grad: feat not 16-byte aligned");
    const bool tensor = a->target != nullptr, analytic = a->joints_hm != nullptr;
    I2R_CHECK_ARG(tensor != analytic, "i2r_head_grad: %s target form given (target tensor, or joints_hm + joints_vis)", tensor ? "more than one" : "no");
    I2R_CHECK_ARG(!analytic || (a->target_weight == nullptr && a->joints_vis != nullptr), "i2r_head_grad: the analytic form takes joints_vis and no target_weight");
    I2R_CHECK_ARG(!analytic || a->sigma > 0.0, "i2r_head_grad: sigma %g", a->sigma);
    I2R_CHECK_ARG(!tensor || a->target_weight || !a->use_target_weight, "i2r_head_grad: use_target_weight without target_weight");
    if (a->n_crops == 0) return I2R_OK;
    I2R_CHECK_ARG(a->feat && a->w && a->bias && a->ws, "i2r_head_grad: null feat / w / bias / workspace");
    I2R_CHECK_ARG(((uintptr_t)a->ws & 7) == 0, "i2r_head_grad: workspace not 8-byte aligned");
    I2R_CHECK_ARG(a->dw && a->db && a->loss && a->sse, "i2r_head_grad: null result pointer");
    const Plan p = make_plan(a->n_crops, a->h * a->w_);
    const dim3 grid((unsigned)p.n_part);
    typedef void (*tile_fn)(const i2r_head_grad_args, const Plan);
    static const tile_fn fns[2][4][2] = {
#define HG_ROW(NF) {{head_grad_tile_k<NF, 2, false>, head_grad_tile_k<NF, 2, true>}, {head_grad_tile_k<NF, 4, false>, head_grad_tile_k<NF, 4, true>}, \
                    {head_grad_tile_k<NF, 6, false>, head_grad_tile_k<NF, 6, true>}, {head_grad_tile_k<NF, 8, false>, head_grad_tile_k<NF, 8, true>}}
        HG_ROW(1), HG_ROW(2)
#undef HG_ROW
    };
    const tile_fn fn = fns[a->joints <= 16 ? 0 : 1][(a->cin - 1) / 32][analytic ? 1 : 0];
    i2r_launch(fn, grid, dim3(64), 0, (hipStream_t)stream, *a, p);
    I2R_CHECK_LAUNCH("i2r_head_grad");
    const int n_colblk = (a->joints * a->cin + a->joints + FIN_COLS - 1) / FIN_COLS;
    i2r_launch(head_grad_finish_k, dim3((unsigned)(n_colblk + 1)), dim3(FIN_NT), 0, (hipStream_t)stream, *a, p, n_colblk);
    I2R_CHECK_LAUNCH("i2r_head_grad (finish)");
    return I2R_OK;
}

#include "i2r_head_normal.h"  // i2r_head_normal, i2r_head_normal_ws_bytes: the closed form of the same fit
