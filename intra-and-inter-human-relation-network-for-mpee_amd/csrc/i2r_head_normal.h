// Head re-fit in closed form: the normal equations of JointsMSELoss in (W, b) on frozen features, collected in one pass (included at the
// end of i2r_head_fit.hip, whose plan, slice_sum, shape_ok and LDS row pitch it shares):
//   i2r_head_normal   A[j] += sum_s tw^2 F~^T F~,  r[j] += sum_s tw^2 F~^T t,  c[j] += sum (tw t)^2,  n += pixels      (F~ = (F, 1))
// The Gram matrix of a crop does not depend on the joint: the tile launch forms it once per part, the finish launch weights it per joint.
//   tile    a workgroup of four waves owns a run of 16-pixel fragments of ONE crop.  Per fragment the 256 threads load the feature rows
//           once (16-byte loads along the channels) into one of two LDS images (one barrier per fragment).  Every wave reads the image
//           back as "lane (channel c, g) takes pixel 4 g + r" -- the B operand of i2r_head_grad's second product -- for every 16-channel
//           block; that read is BOTH operands of a Gram tile (block ci, block cj).  Only tiles with ci <= cj exist; tile p belongs to
//           wave p % 4.  Block cb's share of r = (tw tw t)^T F (i2r_head_grad's second product with tw^2 t in place of g) and of the
//           column sums F^T 1 (the bias row of A) belongs to wave cb % 4.  The targets and tw sit in registers in every wave.
//           The part writes its Gram tiles, r (fp32: at most one crop's pixels), column sums, sum tw^2 t and sum (tw t)^2 (fp64) to the
//           workspace; the first part of a crop also writes the crop's tw.
//   finish  A: a thread owns one element (a, b) -- read at (min, max), so A is symmetric bit for bit -- and every 32nd crop: per crop the
//           parts in ascending order in fp64, then acc[j] += tw^2 * that; the 32 crop slices are added in ascending order by one thread,
//           which does A[j][a][b] += sum.  r, c: as i2r_head_grad's finish (64 interleaved slices of parts, ascending).  n by one thread.
// No floating-point atomics: equal state and equal inputs give equal bits, whatever the workspace held.
#pragma once
#include <utility>

namespace {

constexpr int HN_NT = 256;        // tile launch: four waves
constexpr int HN_WGS = 512;       // parts aimed at: two workgroups per CU.  A part writes its whole Gram matrix (21 tiles = 21.5 KB at cin 96),
                                  // so more parts would outweigh the one read of the features
constexpr int HN_AEL = 32, HN_ASL = FIN_NT / HN_AEL;   // finish, A: 32 elements x 32 crop slices per workgroup

__host__ __device__ constexpr int hn_pairs(int CJ) { return CJ * (CJ + 1) / 2; }
__host__ __device__ constexpr int hn_pair_index(int ci, int cj, int CJ) { return ci * CJ - ci * (ci - 1) / 2 + (cj - ci); }
__host__ __device__ constexpr int hn_pair_i(int p, int CJ) {
    int ci = 0;
    while (p >= CJ - ci) { p -= CJ - ci; ++ci; }
    return ci;
}
__host__ __device__ constexpr int hn_pair_j(int p, int CJ) {
    int ci = 0;
    while (p >= CJ - ci) { p -= CJ - ci; ++ci; }
    return ci + p;
}
// the 16-channel steps compiled in: 2, 4 or 8 (a 6-step instantiation, 21 tiles over four waves, took 480 registers where the 8-step one
// takes 128; cin 96 runs the 8-step kernel, whose tiles and blocks behind cin are skipped by wave-uniform branches)
__host__ __device__ inline int hn_cj_compiled(int cin) { return cin <= 32 ? 2 : cin <= 64 ? 4 : 8; }

__host__ __device__ inline Plan make_nplan(int n_crops, int hw) {
    Plan p;
    p.frags_per_crop = (hw + 15) / 16;
    const long long total = (long long)n_crops * p.frags_per_crop;
    long long fpw = (total + HN_WGS - 1) / HN_WGS;
    if (fpw < 1) fpw = 1;
    if (fpw > p.frags_per_crop) fpw = p.frags_per_crop;
    p.frags_per_wave = (int)fpw;
    p.waves_per_crop = (p.frags_per_crop + p.frags_per_wave - 1) / p.frags_per_wave;
    p.n_part = (long long)n_crops * p.waves_per_crop;
    return p;
}

// workspace: double c [n_part][J], rb [n_part][J], cs [n_part][cin]; float tw [n_crops][J], r [n_part][J][cin], G [n_part][NP][256]
// with NP = the tiles ci <= cj of the cin / 16 channel blocks (21 at cin 96), whatever the instantiation
struct NWs {
    double *c, *rb, *cs;
    float *tw, *r, *G;
    size_t bytes;
};
__host__ __device__ inline NWs make_nws(void* ws, size_t n_part, size_t n_crops, int J, int cin) {
    NWs w;
    const size_t NP = hn_pairs(cin >> 4);
    w.c = reinterpret_cast<double*>(ws);
    w.rb = w.c + n_part * J;
    w.cs = w.rb + n_part * J;
    w.tw = reinterpret_cast<float*>(w.cs + n_part * cin);
    w.r = w.tw + n_crops * J;
    w.G = w.r + n_part * J * cin;
    w.bytes = n_part * (16 * (size_t)J + 8 * (size_t)cin) + 4 * (n_crops * J + n_part * J * cin + n_part * NP * 256);
    return w;
}

// the Gram tiles of one k step: tile P (a compile-time list) belongs to wave P % 4; b[] is the wave's read of every channel block
template <int CJ, int... P>
__device__ __forceinline__ void gram_step(const float (&b)[CJ], f32x4 (&acc)[(hn_pairs(CJ) + 3) / 4], int wv, int cjn, std::integer_sequence<int, P...>) {
    ((wv == P % 4 && hn_pair_j(P, CJ) < cjn ? (void)(acc[P / 4] = mfma16(b[hn_pair_i(P, CJ)], b[hn_pair_j(P, CJ)], acc[P / 4])) : (void)0), ...);
}
// D of a tile: lane (column n, g), register r = row 4 g + r -> G[tile's index among the cjn blocks' tiles][row * 16 + column]
template <int CJ, int... P>
__device__ __forceinline__ void gram_store(float* G, const f32x4 (&acc)[(hn_pairs(CJ) + 3) / 4], int wv, int cjn, int n, int g, std::integer_sequence<int, P...>) {
    ((wv == P % 4 && hn_pair_j(P, CJ) < cjn ? (void)(G[hn_pair_index(hn_pair_i(P, CJ), hn_pair_j(P, CJ), cjn) * 256 + (4 * g + 0) * 16 + n] = acc[P / 4][0],
                                                     G[hn_pair_index(hn_pair_i(P, CJ), hn_pair_j(P, CJ), cjn) * 256 + (4 * g + 1) * 16 + n] = acc[P / 4][1],
                                                     G[hn_pair_index(hn_pair_i(P, CJ), hn_pair_j(P, CJ), cjn) * 256 + (4 * g + 2) * 16 + n] = acc[P / 4][2],
                                                     G[hn_pair_index(hn_pair_i(P, CJ), hn_pair_j(P, CJ), cjn) * 256 + (4 * g + 3) * 16 + n] = acc[P / 4][3])
                                            : (void)0), ...);
}

// NF, ANALYTIC as head_grad_tile_k has them; CJ: hn_cj_compiled
template <int NF, int CJ, bool ANALYTIC>
__global__ __launch_bounds__(HN_NT) void head_normal_tile_k(const i2r_head_normal_args a, const Plan plan) {
    constexpr int NP = hn_pairs(CJ), NA = (NP + 3) / 4, NQ = (CJ + 3) / 4, NB = (CJ + 3) / 4;
    __shared__ __attribute__((aligned(16))) float fl[2][16 * HG_LS];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pn = tid & 15, q = tid >> 4;   // the loader's pixel of the fragment and its first 4-channel group
    const size_t part = blockIdx.x, n_part = (size_t)plan.n_part;
    const int crop = (int)(part / plan.waves_per_crop), wi = (int)(part % plan.waves_per_crop);
    const int J = a.joints, cin = a.cin, cjn = cin >> 4, hw = a.h * a.w_, wd = a.w_;
    const bool use_w = a.use_target_weight != 0;
    const int f0 = wi * plan.frags_per_wave, f1 = min(f0 + plan.frags_per_wave, plan.frags_per_crop);
    const NWs ws = make_nws(a.ws, n_part, (size_t)a.n_crops, J, cin);

    float tw[NF], tw2[NF];
    bool draw[NF], on[NF];
    double mx[NF], my[NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int jn = nf * 16 + n;
        on[nf] = jn < J;
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
            if (wi == 0 && wv == 0 && g == 0) ws.tw[map] = tw[nf];   // the finish launch weights the crop's Gram matrix with it
        }
        tw2[nf] = use_w ? tw[nf] * tw[nf] : 1.f;
    }
    const double two_s2 = 2.0 * a.sigma * a.sigma;
    const bool vec = !ANALYTIC && (hw & 3) == 0 && ((uintptr_t)a.target & 15) == 0;

    f32x4 acc[NA], rw[NF][NB];
    float cs[NB];
    double csum[NF], rb[NF];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        cs[k] = 0.f;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) rw[nf][k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) csum[nf] = rb[nf] = 0.0;

    const float* fcrop = a.feat + (size_t)crop * hw * a.in_cs;
    f32x4 va[NQ];
    auto load_rows = [&](int f) {  // thread (pixel pn, q): in[pixel][4 (q + 16 i) .. + 3]; zero rows behind the crop's last pixel
        const int p = f * 16 + pn;
        const bool ok = f < f1 && p < hw;
        const f32x4* x = reinterpret_cast<const f32x4*>(fcrop + (size_t)(ok ? p : 0) * a.in_cs);
#pragma unroll
        for (int i = 0; i < NQ; ++i) va[i] = (ok && q + 16 * i < cjn * 4) ? x[q + 16 * i] : (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    float tn[NF][4];
    auto load_target = [&](int f) {  // as head_grad_tile_k: lane (joint n, g), the four pixels from 16 f + 4 g
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
        float* img = fl[(f - f0) & 1];
        const int pd = f * 16 + 4 * g;
#pragma unroll
        for (int i = 0; i < NQ; ++i)
            if (q + 16 * i < CJ * 4) *reinterpret_cast<f32x4*>(&img[pn * HG_LS + (q + 16 * i) * 4]) = va[i];
        // tw^2 t (the A operand of r) and the sums that need no feature
        f32x4 gt[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float gg = 0.f;
                if (on[nf] && pd + r < hw) {
                    const float t = tn[nf][r];
                    const float d = use_w ? t * tw[nf] : t;   // i2r_head_grad's loss term at o = 0 (its sign does not reach the square)
                    csum[nf] += (double)(d * d);
                    gg = tw2[nf] * t;
                    rb[nf] += (double)gg;
                }
                gt[nf][r] = gg;
            }
        }
        __syncthreads();  // the feature rows are in this image; the other one was read a fragment ago, before this barrier
        load_rows(f + 1);
        load_target(f + 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float b[CJ];
#pragma unroll
            for (int cb = 0; cb < CJ; ++cb) b[cb] = cb < cjn ? img[(4 * g + r) * HG_LS + cb * 16 + n] : 0.f;
            gram_step<CJ>(b, acc, wv, cjn, std::make_integer_sequence<int, NP>{});
#pragma unroll
            for (int cb = 0; cb < CJ; ++cb)
                if ((cb & 3) == wv && cb < cjn) {
                    cs[cb >> 2] += b[cb];
#pragma unroll
                    for (int nf = 0; nf < NF; ++nf) rw[nf][cb >> 2] = mfma16(gt[nf][r], b[cb], rw[nf][cb >> 2]);
                }
        }
    }

    gram_store<CJ>(ws.G + part * (size_t)hn_pairs(cjn) * 256, acc, wv, cjn, n, g, std::make_integer_sequence<int, NP>{});
    // D of r: lane (channel c = n, g), register r = joint 16 nf + 4 g + r; the column sums: the four pixel groups in ascending order
    float* pr = ws.r + part * (size_t)J * cin;
#pragma unroll
    for (int cb = 0; cb < CJ; ++cb)
        if ((cb & 3) == wv && cb < cjn) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int jq = nf * 16 + 4 * g + r;
                    if (jq < J) pr[(size_t)jq * cin + cb * 16 + n] = rw[nf][cb >> 2][r];
                }
            const double v = (double)cs[cb >> 2];
            double s = __shfl(v, n);
#pragma unroll
            for (int k = 1; k < 4; ++k) s += __shfl(v, n + 16 * k);
            if (g == 0) ws.cs[part * cin + cb * 16 + n] = s;
        }
    if (wv == 0) {
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            double s = __shfl(csum[nf], n), d = __shfl(rb[nf], n);
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                s += __shfl(csum[nf], n + 16 * k);
                d += __shfl(rb[nf], n + 16 * k);
            }
            if (g == 0 && on[nf]) {
                ws.c[part * J + nf * 16 + n] = s;
                ws.rb[part * J + nf * 16 + n] = d;
            }
        }
    }
}

// Workgroups [0, n_ablk): 32 elements of A each; [n_ablk, n_ablk + n_colblk): 16 columns of (r | r's bias entry | c) each
__global__ __launch_bounds__(FIN_NT) void head_normal_finish_k(const i2r_head_normal_args a, const Plan plan, int n_ablk) {
    __shared__ double red[FIN_SLICES][FIN_COLS + 1];
    __shared__ double ared[HN_ASL][HN_AEL + 1];
    const int J = a.joints, cin = a.cin, co = a.cin_out, ld = a.ld, tid = threadIdx.x;
    const size_t n_part = (size_t)plan.n_part;
    const NWs ws = make_nws(a.ws, n_part, (size_t)a.n_crops, J, cin);
    if ((int)blockIdx.x >= n_ablk) {
        const int e = tid % FIN_COLS, k = tid / FIN_COLS, JC = J * cin;
        const int col = ((int)blockIdx.x - n_ablk) * FIN_COLS + e;
        double s = 0.0;
        if (col < JC) s = slice_sum(ws.r + col, (size_t)JC, k, FIN_SLICES, n_part);
        else if (col < JC + J) s = slice_sum(ws.rb + (col - JC), (size_t)J, k, FIN_SLICES, n_part);
        else if (col < JC + 2 * J) s = slice_sum(ws.c + (col - JC - J), (size_t)J, k, FIN_SLICES, n_part);
        red[k][e] = s;
        __syncthreads();
        if (k == 0 && col < JC + 2 * J) {
            double tot = 0.0;
            for (int kk = 0; kk < FIN_SLICES; ++kk) tot += red[kk][e];
            if (col < JC) {
                const int j = col / cin, c = col % cin;
                if (c < co) a.r[(size_t)j * ld + c] += tot;   // (a channel behind cin_out is the caller's zero padding: no state)
            } else if (col < JC + J) {
                a.r[(size_t)(col - JC) * ld + co] += tot;
            } else {
                a.c[col - JC - J] += tot;
            }
        }
        if ((int)blockIdx.x == n_ablk && tid == 0) *a.n += (int64_t)a.n_crops * a.h * a.w_;
        return;
    }
    const int el = tid % HN_AEL, sl = tid / HN_AEL;
    const int e = blockIdx.x * HN_AEL + el, side = co + 1;
    const bool valid = e < side * side;
    const int ra = valid ? e / side : 0, rc = valid ? e % side : 0, lo = min(ra, rc), hi = max(ra, rc);
    const int NP = hn_pairs(cin >> 4), wpc = plan.waves_per_crop;
    const bool count = hi == co && lo == co, colsum = hi == co && lo < co;
    const size_t goff = count || colsum ? 0 : (size_t)hn_pair_index(lo >> 4, hi >> 4, cin >> 4) * 256 + (lo & 15) * 16 + (hi & 15);
    const bool use_w = a.use_target_weight != 0;
    double acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = 0.0;
    if (valid) {
        for (int s = sl; s < a.n_crops; s += HN_ASL) {
            double gs = 0.0;   // the crop's own sum: its parts in ascending order
            if (count) {
                gs = (double)a.h * (double)a.w_;
            } else if (colsum) {
                const double* p = ws.cs + (size_t)s * wpc * cin + lo;
#pragma unroll 4
                for (int i = 0; i < wpc; ++i) gs += p[(size_t)i * cin];
            } else {
                const float* p = ws.G + (size_t)s * wpc * NP * 256 + goff;
#pragma unroll 4
                for (int i = 0; i < wpc; ++i) gs += (double)p[(size_t)i * NP * 256];
            }
            const float* twr = ws.tw + (size_t)s * J;
#pragma unroll
            for (int j = 0; j < 32; ++j)
                if (j < J) {
                    const double t = use_w ? (double)twr[j] : 1.0;
                    acc[j] += (t * t) * gs;
                }
        }
    }
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (j < J) {  // (the same for the whole workgroup)
            ared[sl][el] = acc[j];
            __syncthreads();
            if (sl == 0 && valid) {
                double tot = 0.0;
                for (int kk = 0; kk < HN_ASL; ++kk) tot += ared[kk][el];
                a.A[((size_t)j * ld + ra) * ld + rc] += tot;
            }
            __syncthreads();
        }
}

}  // namespace

extern "C" int i2r_head_normal_ws_bytes(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t* bytes) {
    I2R_CHECK_ARG(bytes, "i2r_head_normal_ws_bytes: null result pointer");
    I2R_CHECK_ARG(shape_ok(n_crops, h, w_, cin, joints), "i2r_head_normal_ws_bytes: %d crops, %d x %d, cin=%d, joints=%d", n_crops, h, w_, cin, joints);
    if (n_crops == 0) {
        *bytes = 0;
        return I2R_OK;
    }
    const Plan p = make_nplan(n_crops, h * w_);
    *bytes = (int64_t)make_nws(nullptr, (size_t)p.n_part, (size_t)n_crops, joints, cin).bytes;
    return I2R_OK;
}

extern "C" int i2r_head_normal(const i2r_head_normal_args* a, void* stream) {
    I2R_CHECK_ARG(a, "i2r_head_normal: null args");
    I2R_CHECK_ARG(shape_ok(a->n_crops, a->h, a->w_, a->cin, a->joints), "i2r_head_normal: %d crops, %d x %d, cin=%d (a multiple of 16 in [16, 128]), joints=%d (1 .. 32)",
                  a->n_crops, a->h, a->w_, a->cin, a->joints);
    I2R_CHECK_ARG(a->cin <= a->in_cs && a->in_cs % 4 == 0, "i2r_head_normal: cin=%d in_cs=%d", a->cin, a->in_cs);
    I2R_CHECK_ARG(a->cin_out >= 1 && a->cin_out <= a->cin && a->ld > a->cin_out, "i2r_head_normal: cin_out=%d (1 .. cin=%d), ld=%d (> cin_out)", a->cin_out, a->cin, a->ld);
    I2R_CHECK_ARG(((uintptr_t)a->feat & 15) == 0, "i2r_head_normal: feat not 16-byte aligned");
    const bool tensor = a->target != nullptr, analytic = a->joints_hm != nullptr;
    I2R_CHECK_ARG(tensor != analytic, "i2r_head_normal: %s target form given (target tensor, or joints_hm + joints_vis)", tensor ? "more than one" : "no");
    I2R_CHECK_ARG(!analytic || (a->target_weight == nullptr && a->joints_vis != nullptr), "i2r_head_normal: the analytic form takes joints_vis and no target_weight");
    I2R_CHECK_ARG(!analytic || a->sigma > 0.0, "i2r_head_normal: sigma %g", a->sigma);
    I2R_CHECK_ARG(!tensor || a->target_weight || !a->use_target_weight, "i2r_head_normal: use_target_weight without target_weight");
    if (a->n_crops == 0) return I2R_OK;
    I2R_CHECK_ARG(a->feat && a->ws, "i2r_head_normal: null feat / workspace");
    I2R_CHECK_ARG(((uintptr_t)a->ws & 7) == 0, "i2r_head_normal: workspace not 8-byte aligned");
    I2R_CHECK_ARG(a->A && a->r && a->c && a->n, "i2r_head_normal: null state pointer");
    I2R_CHECK_ARG((((uintptr_t)a->A | (uintptr_t)a->r | (uintptr_t)a->c | (uintptr_t)a->n) & 7) == 0, "i2r_head_normal: state not 8-byte aligned");
    const Plan p = make_nplan(a->n_crops, a->h * a->w_);
    typedef void (*tile_fn)(const i2r_head_normal_args, const Plan);
    static const tile_fn fns[2][3][2] = {
#define HN_ROW(NF) {{head_normal_tile_k<NF, 2, false>, head_normal_tile_k<NF, 2, true>}, {head_normal_tile_k<NF, 4, false>, head_normal_tile_k<NF, 4, true>}, \
                    {head_normal_tile_k<NF, 8, false>, head_normal_tile_k<NF, 8, true>}}
        HN_ROW(1), HN_ROW(2)
#undef HN_ROW
    };
    const int cjc = hn_cj_compiled(a->cin);
    const tile_fn fn = fns[a->joints <= 16 ? 0 : 1][cjc == 2 ? 0 : cjc == 4 ? 1 : 2][analytic ? 1 : 0];
    i2r_launch(fn, dim3((unsigned)p.n_part), dim3(HN_NT), 0, (hipStream_t)stream, *a, p);
    I2R_CHECK_LAUNCH("i2r_head_normal");
    const int side = a->cin_out + 1;
    const int n_ablk = (side * side + HN_AEL - 1) / HN_AEL, n_colblk = (a->joints * a->cin + 2 * a->joints + FIN_COLS - 1) / FIN_COLS;
    i2r_launch(head_normal_finish_k, dim3((unsigned)(n_ablk + n_colblk)), dim3(FIN_NT), 0, (hipStream_t)stream, *a, p, n_ablk);
    I2R_CHECK_LAUNCH("i2r_head_normal (finish)");
    return I2R_OK;
}
