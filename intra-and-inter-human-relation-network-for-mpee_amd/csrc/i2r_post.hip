// The steps that follow the forward in the reference's validate() loop (NEXT #1/#2), on device:
//   i2r_flip_merge  flip-test merge: (y + flip_back(y_flipped)) * 0.5        lib/core/function.py:142-162, utils/transforms.py:16-30
//   i2r_decode      heatmap -> keypoints (DarkPose decode)                   lib/core/inference.py:20-112, utils/transforms.py:50-101
//   i2r_joint_tokens  heatmap -> arg-max points and the query-token tables of i2r_attn_query_maps   lib/core/inference.py:20-48, visualize.py:194-196
// All are tiny, HBM/LDS-bound kernels; they remove the D2H copy of every heatmap and a Python double loop over S x J.
#include "i2r_common.h"

namespace {

__global__ __launch_bounds__(256) void flip_merge_k(const float* __restrict__ y, const float* __restrict__ yf,
                                                    const int* __restrict__ jmap, float* __restrict__ out, int n, int J, int h,
                                                    int w) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)n * J * h * w) return;
    const int x = (int)(gid % w);
    const long long r = gid / w;
    const int yy = (int)(r % h);
    const int j = (int)((r / h) % J);
    const int s = (int)(r / ((long long)h * J));
    const float b = yf[(((size_t)s * J + jmap[j]) * h + yy) * w + (w - 1 - x)];
    out[gid] = (y[gid] + b) * 0.5f;
}

struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ ArgMax amax2(ArgMax a, ArgMax b) {  // np.argmax: first occurrence wins ties
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

// cv2.getGaussianKernel(ksize, sigma <= 0) does not evaluate the Gaussian for odd ksize <= 7: it returns a fixed table
// (small_gaussian_tab, OpenCV modules/imgproc/src/smooth.dispatch.cpp); only from ksize 9 on does it use sigma = 0.3*((ksize-1)*0.5-1)+0.8.
// Row (ksize-1)/2, indexed by the distance from the centre tap.  ksize 1 is the identity: "no blur" (the reference itself cannot run it,
// its dr[0:-0] is empty).  Taken from the OpenCV source; not compared against a cv2 run.
__device__ const float kSmallGaussian[4][4] = {{1.f, 0.f, 0.f, 0.f},
                                               {0.5f, 0.25f, 0.f, 0.f},
                                               {0.375f, 0.25f, 0.0625f, 0.f},
                                               {0.28125f, 0.21875f, 0.109375f, 0.03125f}};

// one workgroup per (crop, joint). LDS: A[h*w] (heatmap, later the blurred map), B[h*w] (row-filtered)
__global__ __launch_bounds__(256) void decode_k(const float* __restrict__ hm, const float* __restrict__ center,
                                                const float* __restrict__ scale, float* __restrict__ preds, float* __restrict__ maxvals,
                                                int J, int h, int w, int ksize, int transform_back) {
    extern __shared__ float sm[];
    float* A = sm;
    float* B = sm + h * w;
    __shared__ ArgMax red[4];
    __shared__ float redf[4];
    __shared__ float gk[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sj = blockIdx.x;
    const int hw = h * w;
    const float* src = hm + (size_t)sj * hw;
    const int border = (ksize - 1) / 2;
    if (tid < ksize) {  // cv2.getGaussianKernel(ksize, sigma <= 0), see kSmallGaussian
        if (ksize <= 7) {
            const int d = tid < border ? border - tid : tid - border;
            gk[tid] = kSmallGaussian[border][d];
        } else {  // sigma = 0.3*((ksize-1)*0.5 - 1) + 0.8, normalised to sum 1
            const double sigma = 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8;
            double sum = 0.0;
            for (int k = 0; k < ksize; ++k) sum += exp(-0.5 * (k - border) * (k - border) / (sigma * sigma));
            gk[tid] = (float)(exp(-0.5 * (tid - border) * (tid - border) / (sigma * sigma)) / sum);
        }
    }
    ArgMax am = {-__builtin_inff(), 0x7fffffff};
    for (int i = tid; i < hw; i += 256) {
        const float v = src[i];
        A[i] = v;
        am = amax2(am, ArgMax{v, i});
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = amax2(am, ArgMax{__shfl_xor(am.v, o), __shfl_xor(am.i, o)});
    if (lane == 0) red[wave] = am;
    __syncthreads();
    am = amax2(amax2(red[0], red[1]), amax2(red[2], red[3]));
    const float origin_max = am.v;
    // row filter (zero padding == the reference's explicit zero border of width (ksize-1)/2)
    for (int i = tid; i < hw; i += 256) {
        const int y = i / w, x = i - y * w;
        float acc = 0.f;
        for (int k = 0; k < ksize; ++k) {
            const int xx = x + k - border;
            if (xx >= 0 && xx < w) acc = fmaf(gk[k], A[y * w + xx], acc);
        }
        B[i] = acc;
    }
    __syncthreads();
    float bm = -__builtin_inff();
    for (int i = tid; i < hw; i += 256) {  // column filter
        const int y = i / w, x = i - y * w;
        float acc = 0.f;
        for (int k = 0; k < ksize; ++k) {
            const int yy = y + k - border;
            if (yy >= 0 && yy < h) acc = fmaf(gk[k], B[yy * w + x], acc);
        }
        A[i] = acc;
        bm = fmaxf(bm, acc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bm = fmaxf(bm, __shfl_xor(bm, o));
    if (lane == 0) redf[wave] = bm;
    __syncthreads();
    if (tid != 0) return;
    bm = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    const float rescale = origin_max / bm;                       // hm *= origin_max / max(blurred)
    auto L = [&](int y, int x) { return logf(fmaxf(A[y * w + x] * rescale, 1e-10f)); };  // log(max(hm, 1e-10))
    float cx = (float)(am.i % w), cy = floorf((float)am.i / (float)w);
    if (!(origin_max > 0.f)) { cx = 0.f; cy = 0.f; }             // pred_mask (inference.py:42-45)
    const int px = (int)cx, py = (int)cy;
    if (1 < px && px < w - 2 && 1 < py && py < h - 2) {         // taylor (inference.py:51-70)
        const float dx = 0.5f * (L(py, px + 1) - L(py, px - 1));
        const float dy = 0.5f * (L(py + 1, px) - L(py - 1, px));
        const float dxx = 0.25f * (L(py, px + 2) - 2.f * L(py, px) + L(py, px - 2));
        const float dxy = 0.25f * (L(py + 1, px + 1) - L(py - 1, px + 1) - L(py + 1, px - 1) + L(py - 1, px - 1));
        const float dyy = 0.25f * (L(py + 2, px) - 2.f * L(py, px) + L(py - 2, px));
        const float det = dxx * dyy - dxy * dxy;
        if (det != 0.f) {  // offset = -H^-1 g
            cx += -(dyy * dx - dxy * dy) / det;
            cy += -(-dxy * dx + dxx * dy) / det;
        }
    }
    if (transform_back) {  // inverse of the crop affine with rot = 0: pure scale about the centres (transforms.py:50-90)
        const int s = sj / J;
        const float r = (scale[s * 2] * 200.f - 1.f) / (float)(w - 1);
        cx = center[s * 2] + (cx - 0.5f * (float)(w - 1)) * r;
        cy = center[s * 2 + 1] + (cy - 0.5f * (float)(h - 1)) * r;
    }
    preds[(size_t)sj * 2] = cx;
    preds[(size_t)sj * 2 + 1] = cy;
    maxvals[sj] = origin_max;
}

// get_max_preds (inference.py:20-48) of every map -> points, maxvals and the query-token tables of the encoder stacks.  One wave per
// (crop, joint) map, four maps per workgroup; the arg-max is decode_k's (amax2, the same butterfly), so the two agree on every tie.
struct TokenTables {
    i2r_token_table t[I2R_MAX_TOKEN_TABLES];
    int n;
};
__global__ __launch_bounds__(256) void joint_tokens_k(const float* __restrict__ hm, float* __restrict__ points, float* __restrict__ maxvals,
                                                      TokenTables tabs, int n_maps, int J, int hw, int w, int in_stride) {
    const int lane = threadIdx.x & 63;
    const long long map = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (map >= n_maps) return;  // (wave-uniform)
    const float* src = hm + (size_t)map * hw;
    ArgMax am = {-__builtin_inff(), 0x7fffffff};
    for (int i = lane; i < hw; i += 64) am = amax2(am, ArgMax{src[i], i});
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = amax2(am, ArgMax{__shfl_xor(am.v, o), __shfl_xor(am.i, o)});
    if (lane != 0) return;
    int px = 0, py = 0;
    if (am.v > 0.f) { px = am.i % w; py = am.i / w; }  // pred_mask (inference.py:42-45); a map of NaNs keeps the sentinel index: (0, 0) too
    px *= in_stride;
    py *= in_stride;
    if (points) {
        points[(size_t)map * 2] = (float)px;
        points[(size_t)map * 2 + 1] = (float)py;
    }
    if (maxvals) maxvals[map] = am.v;
    const int s = (int)(map / J), j = (int)(map - (long long)s * J);
    for (int t = 0; t < tabs.n; ++t) {
        const i2r_token_table& T = tabs.t[t];
        const int g = T.crop_group[s], slot = T.crop_slot[s];
        if (g < 0 || g >= T.n_grp || slot < 0 || ((long long)slot + 1) * J > T.K) continue;  // (a wrong device table costs entries, never a store outside)
        const int row = min(py / T.down, T.fh - 1), col = min(px / T.down, T.fw - 1);
        T.tokens[(size_t)g * T.K + slot * J + j] = slot * T.fh * T.fw + row * T.fw + col;
    }
}

}  // namespace

extern "C" int i2r_joint_tokens(const i2r_joint_tokens_args* a, void* stream) {
    I2R_CHECK_ARG(a && a->heatmaps, "i2r_joint_tokens: null pointer");
    I2R_CHECK_ARG(a->n_crops >= 1 && a->joints >= 1 && a->hh >= 1 && a->hw >= 1 && a->in_stride >= 1,
                  "i2r_joint_tokens: n_crops=%d joints=%d heatmap %dx%d in_stride=%d", a->n_crops, a->joints, a->hh, a->hw, a->in_stride);
    I2R_CHECK_ARG(a->n_tables >= 0 && a->n_tables <= I2R_MAX_TOKEN_TABLES, "i2r_joint_tokens: n_tables=%d (0 .. %d)", a->n_tables,
                  I2R_MAX_TOKEN_TABLES);
    I2R_CHECK_ARG(a->n_tables > 0 || a->points || a->maxvals, "i2r_joint_tokens: null pointer (no output)");
    const long long n_maps = (long long)a->n_crops * a->joints, pix = (long long)a->hh * a->hw;
    I2R_CHECK_ARG(pix <= 0x7fffffffLL && (long long)(a->hh > a->hw ? a->hh : a->hw) * a->in_stride <= 0x7fffffffLL,
                  "i2r_joint_tokens: heatmap %dx%d at in_stride=%d exceeds the index range", a->hh, a->hw, a->in_stride);
    I2R_CHECK_ARG(n_maps <= 0x7fffffffLL, "i2r_joint_tokens: %lld maps exceed the grid limit", n_maps);
    TokenTables tabs;
    tabs.n = a->n_tables;
    for (int t = 0; t < I2R_MAX_TOKEN_TABLES; ++t) {
        tabs.t[t] = t < a->n_tables ? a->table[t] : i2r_token_table{};
        if (t >= a->n_tables) continue;
        const i2r_token_table& T = a->table[t];
        I2R_CHECK_ARG(T.tokens && T.crop_group && T.crop_slot, "i2r_joint_tokens: null pointer (table %d)", t);
        I2R_CHECK_ARG(T.n_grp >= 1 && T.fh >= 1 && T.fw >= 1 && T.down >= 1, "i2r_joint_tokens: table %d: n_grp=%d token map %dx%d down=%d", t,
                      T.n_grp, T.fh, T.fw, T.down);
        I2R_CHECK_ARG(T.K >= a->joints, "i2r_joint_tokens: table %d: K=%d < joints=%d", t, T.K, a->joints);
        I2R_CHECK_ARG((long long)T.n_grp * T.K <= 0x7fffffffLL && (long long)(T.K / a->joints) * T.fh * T.fw <= 0x7fffffffLL,
                      "i2r_joint_tokens: table %d: n_grp=%d K=%d, %d persons of %dx%d tokens exceed the index range", t, T.n_grp, T.K,
                      T.K / a->joints, T.fh, T.fw);
    }
    for (int t = 0; t < a->n_tables; ++t) {  // -1 = skip: what no crop writes
        const hipError_t e = hipMemsetAsync(a->table[t].tokens, 0xFF, (size_t)a->table[t].n_grp * a->table[t].K * sizeof(int32_t), (hipStream_t)stream);
        if (e != hipSuccess) {
            i2r_set_error("i2r_joint_tokens: memset of table %d: %s", t, hipGetErrorString(e));
            return I2R_E_LAUNCH;
        }
    }
    i2r_launch(joint_tokens_k, dim3((unsigned)((n_maps + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a->heatmaps, a->points, a->maxvals, tabs,
               (int)n_maps, a->joints, (int)pix, a->hw, a->in_stride);
    I2R_CHECK_LAUNCH("i2r_joint_tokens");
    return I2R_OK;
}

extern "C" int i2r_flip_merge(const float* y, const float* y_flipped, const int32_t* joint_map, float* out, int32_t n, int32_t joints,
                              int32_t h, int32_t w, void* stream) {
    I2R_CHECK_ARG(y && y_flipped && joint_map && out, "i2r_flip_merge: null pointer");
    I2R_CHECK_ARG(n >= 0 && joints >= 1 && h >= 1 && w >= 1, "i2r_flip_merge: n %d joints %d heatmap %dx%d", n, joints, h, w);
    if (n == 0) return I2R_OK;
    const long long tot = (long long)n * joints * h * w;
    I2R_CHECK_ARG((tot + 255) / 256 <= 0x7fffffffLL, "i2r_flip_merge: %lld elements exceed the grid limit", tot);
    i2r_launch(flip_merge_k, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, y_flipped, joint_map,
                       out, n, joints, h, w);
    I2R_CHECK_LAUNCH("i2r_flip_merge");
    return I2R_OK;
}

extern "C" int i2r_decode(const float* heatmaps, const float* center, const float* scale, float* preds, float* maxvals, int32_t n,
                          int32_t joints, int32_t h, int32_t w, int32_t blur_kernel, int32_t transform_back, void* stream) {
    I2R_CHECK_ARG(heatmaps && preds && maxvals && (!transform_back || (center && scale)), "i2r_decode: null pointer");
    I2R_CHECK_ARG(blur_kernel >= 1 && blur_kernel <= 31 && (blur_kernel & 1), "i2r_decode: blur kernel %d", blur_kernel);
    I2R_CHECK_ARG(n >= 0 && joints >= 1 && h >= 1 && w > 1, "i2r_decode: n %d joints %d heatmap %dx%d", n, joints, h, w);
    I2R_CHECK_ARG((long long)n * joints <= 0x7fffffffLL, "i2r_decode: %lld maps exceed the grid limit", (long long)n * joints);
    I2R_CHECK_ARG((long long)h * w <= 150 * 1024 / 8, "i2r_decode: heatmap %dx%d too large", h, w);
    if (n == 0) return I2R_OK;
    const size_t lds = (size_t)2 * h * w * sizeof(float);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    i2r_launch(decode_k, dim3((unsigned)(n * joints)), dim3(256), lds, (hipStream_t)stream, heatmaps, center, scale, preds,
                       maxvals, joints, h, w, blur_kernel, transform_back);
    I2R_CHECK_LAUNCH("i2r_decode");
    return I2R_OK;
}
