/*
 * i2r_hip.h -- C-ABI of the MI355X-native I2R-Net inference hot path (libi2r_hip.so, gfx950 only).
 *
 * The reference (leijue222/Intra-and-Inter-Human-Relation-Network-for-MPEE) has NO FFI on this path: its
 * boundary is the Python module contract  models.<MODEL.NAME>.get_pose_net(cfg, is_train) ->
 * nn.Module,  called as  model(input, pos_mask, length)  (lib/core/function.py:135, tools/test.py:87).
 * Every arithmetic op behind that call is issued by torch.nn modules.  This header declares the
 * entry points a maintainer binds instead (ctypes stub in INTEGRATION.md); each one names the
 * reference construct it replaces.
 *
 * Conventions
 *  - plain pointers + sizes only; all pointers are DEVICE pointers owned by the caller (inputs, outputs,
 *    packed weights, workspace); the library allocates nothing and keeps no global state.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous and
 *    re-entrant per stream.
 *  - return 0 on success, negative I2R_E_* otherwise; i2r_last_error() gives a thread-local message.
 *  - activations are fp32 NHWC ("pixel-major, channel-minor") with an explicit channel stride; the
 *    boundary tensors keep the reference's NCHW fp32 layout (i2r_stem_conv reads NCHW, i2r_head writes NCHW).
 */
#ifndef I2R_HIP_H
#define I2R_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when an existing entry point, struct layout or op code changes.  Entry points that are only ADDED (i2r_joint_targets,
 * i2r_val_metrics, i2r_val_combine, i2r_oks_match, i2r_oks_accumulate) do not bump it: no existing struct changes with them, and a binding built
 * against the older header keeps working with the newer library. */
#define I2R_ABI_VERSION 17

/* The library is built with -fvisibility=hidden: the entry points declared in this header (marked I2R_API) are its ONLY exported
 * symbols (tests/test_host.py holds the header, the dynamic symbol table and cabi.EXPORTS equal). */
#define I2R_API __attribute__((visibility("default")))

#define I2R_OK 0
#define I2R_E_ARG (-1)      /* bad argument (shape / alignment / unsupported combination) */
#define I2R_E_LAUNCH (-2)   /* HIP launch failure */
#define I2R_E_NODEV (-3)    /* no gfx950 device */

#define I2R_MAX_TAPS 9

/* ------------------------------------------------------------------------------------------------
 * i2r_conv_desc -- one fused  conv (implicit GEMM on fp32 MFMA) [+ folded BN bias] [+ residual(s)]
 * [+ ReLU] [+ nearest-upsample scatter]  launch.
 * Replaces: nn.Conv2d + nn.BatchNorm2d(eval) + nn.ReLU / residual add / nn.Upsample(nearest) /
 * the sum of HighResolutionModule.forward (reference lib/models/interformer_pureMulti.py:50-66,
 * 87-107, 332-410), nn.ConvTranspose2d(k4,s2,p1) split into its 4 output-parity 2x2 convs
 * (interformer_pureMulti.py:648-673, interformer.py:84-122), and nn.Linear on token matrices
 * (a 1x1 conv over [T,1,1,C]).
 *
 *   acc[p, co] = sum_{t < ntaps} sum_{ci < cin}  IN[n, oy*stride + iy0 + dy[t], ox*stride + ix0 + dx[t], ci]
 *                                               * W[t][ci][co]              (IN = in (+ in2 if given))
 *   v = acc + bias[co];  v += res1[dst, co] (if res1);  v += res2[dst, co] (if res2);  relu (if relu);
 *   v += res_post[dst, co] (if res_post: residual added AFTER the ReLU, interformer.py:315)
 *   dst pixels: (oy*out_step + out_off_y + ry, ox*out_step + out_off_x + rx) for ry,rx < rep
 *
 * Packed weight layout ("k4"): float w[ntaps][cin/4][cout_pad][4]  (cin % 16 == 0, cout_pad % 16 == 0,
 * zero-filled beyond cout); bias[cout_pad].
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2r_conv_desc {
    const float* in;     /* [n_img, in_h, in_w, in_cs] */
    const float* in2;    /* optional second input added element-wise while staging (same geometry) */
    const float* w;      /* packed k4 weights */
    const float* bias;   /* [cout_pad] */
    const float* res1;   /* optional, laid out like out */
    const float* res2;   /* optional, laid out like out */
    const float* res_post; /* optional, laid out like out, added after the ReLU */
    float* out;          /* [n_img, out_h, out_w, out_cs] */
    int32_t n_img;
    int32_t in_h, in_w, in_cs;     /* in_cs = channel stride (floats) per input pixel */
    int32_t cin;                   /* multiple of 16, <= in_cs */
    int32_t conv_h, conv_w;        /* logical conv output grid (oy, ox ranges) */
    int32_t out_h, out_w, out_cs;  /* destination tensor geometry */
    int32_t cout, cout_pad;        /* real / padded output channels */
    int32_t stride;                /* 1 or 2 */
    int32_t iy0, ix0;              /* input coordinate of tap offset (0,0) for output (0,0): -pad */
    int32_t ntaps;
    int32_t dy[I2R_MAX_TAPS], dx[I2R_MAX_TAPS];
    int32_t out_step, out_off_y, out_off_x, rep;
    int32_t relu;                  /* activation: 0 none, 1 ReLU, 2 exact-erf GELU */
    int32_t tile_h, tile_w;        /* output tile per workgroup (0 = let the library choose) */
    int32_t ck;                    /* input channels staged in LDS per pass (0 = choose) */
    int32_t wn;                    /* waves along cout in the 4-wave workgroup: 1, 2 or 4 (0 = choose) */
    int32_t mt;                    /* 16-pixel fragments per wave, 1..4 (0 = derive from the tile) */
    int32_t dtype;                 /* MFMA operand type: 0 fp32 (w = k4 fp32), 1 bf16, 2 f16 (w = "k8" [tap][cin32/8][cout_pad][8],
                                      cin zero-padded to a multiple of 32; accumulate fp32) */
    int32_t in_f16, out_f16;       /* dtype != 0 only: activation STORAGE of `in` / of `out`, res1, res2 and res_post -- 0 fp32,
                                      1 = 16 bit of the operand type (bf16 / f16; the pointers then address 2-byte elements, all strides
                                      and offsets stay in elements).  The conv towers of the 16-bit modes keep their maps in 16 bit. */
    int32_t algo;                  /* 0 = direct implicit GEMM.  1 = Winograd F(2x2, 3x3): dtype 0, dense 3x3 taps with iy0 = ix0 = -1, stride 1,
                                      rep = out_step = 1, no in2; `w` then holds the TRANSFORMED weights U = G g G^T in the k4 layout with the 16
                                      Winograd positions (row-major 4x4) in place of the taps: float w[16][cin/4][cout_pad][4].  tile_w selects the
                                      fragment shape (16 Winograd tiles = 64 output pixels): 16, 8 or 4 pixels wide (0 = choose); mt = fragments per
                                      workgroup (0 or 1: one).  2.25x fewer matrix-pipe operations than algo 0 for the same sum. */
    int32_t t1_shift, t2_shift;    /* fused input (below): log2 of the up-sampling factors of t1 / t2, 1 or 2 */
    const float* t1;               /* algo 1 only, optional "fused input": the conv's input is  ReLU((in + up(t1)) + up(t2))  instead of `in` --  */
    const float* t2;               /*   the closing pass of an HRNet fuse layer (i2r_fuse_up_add, same summation order) folded into the staging. */
    float* y;                      /*   t1 / t2 (optional): [n_img, in_h >> shift, in_w >> shift, in_cs], nearest-neighbour up-sampled; the map is
                                        also written to y (required with t1; laid out like `in`, in_cs == cin) for the consumers after this conv.
                                        y must not alias in, t1, t2, out or a residual.  All null = none. */
    int32_t seq;                   /* algo 1 only: fragments (x mt) a workgroup runs one after the other on one set-up.  0 = the library chooses
                                      (from the passes and workgroup counts of all members of the launch), 1 = one fragment per workgroup,
                                      n = 2..8 forces n.  The results do not depend on it, bit for bit.  Other algorithms ignore it. */
} i2r_conv_desc;

I2R_API int i2r_conv(const i2r_conv_desc* d, void* stream);

/* i2r_conv_grouped -- up to I2R_MAX_GROUP independent convolutions in ONE launch ("horizontal fusion"): the
 * parallel branches of a HighResolutionModule (interformer_pureMulti.py:396-397) and the same-depth terms of its
 * fuse sums (:401-408) have no mutual dependencies, and individually the low-resolution ones cannot fill 256 CUs.
 * All descriptors must resolve to the same fragment blocking: cout_pad/16 divisible by the same NT, same mt. */
#define I2R_MAX_GROUP 4
/* block_map (optional, device int32[map_len]): dispatch order of the workgroups, entry = (member << 24) | index of
 * the workgroup within that member; map_len must equal the total workgroup count
 * (sum over members of n_img * ceil(conv_h/tile_h) * ceil(conv_w/tile_w) * cout_blocks; an algo 1 member counts runs of `seq`
 * fragments instead of fragments -- i2r_conv_grid reports the count). */
I2R_API int i2r_conv_grouped(const i2r_conv_desc* const* descs, int32_t n, const int32_t* block_map, int32_t map_len,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * i2r_stem_conv -- first 3x3 stride-2 pad-1 conv of a tower (cin = 1..4) + folded BN + ReLU, reading the
 * boundary NCHW fp32 tensor and writing NHWC.
 * Replaces: conv1+bn1+relu (interformer_pureMulti.py:677-679) and PositionEmbeddingImage conv1+bn1+relu
 * (position_embedding.py:99-101).   w: float[9][cin][cout], bias[cout]; cout % 16 == 0.
 * n_src: the input holds n_src images; output images n_src..n_img-1 (n_img == 2*n_src) are computed from the
 * horizontally mirrored input (np.flip(input, 3) of the flip test, lib/core/function.py:145-150); n_src == n_img: none.
 * n_valid (1..n_src): the input tensor really holds n_valid images; output slots n_valid..n_src-1 (capacity padding of a
 * pre-built launch program) are computed from image n_valid-1 and are the caller's to drop.
 * ------------------------------------------------------------------------------------------------ */
I2R_API int i2r_stem_conv(const float* in_nchw, const float* w, const float* bias, float* out_nhwc, int32_t n_img,
                  int32_t cin, int32_t in_h, int32_t in_w, int32_t cout, int32_t out_cs, int32_t n_src, int32_t n_valid,
                  int32_t out_dt /* storage of out: 0 fp32, 1 bf16, 2 f16 (see i2r_conv_desc.in_f16) */, void* stream);

/* i2r_pe_res_stem -- front end of PositionEmbeddingImage mode 'res' (lib/models/position_embedding.py:14-17,93-95):
 * conv_pre (nn.Conv2d(1, 3, 3, padding=1, bias=False)) followed by torchvision resnet18's conv1 (3 -> 64, 7x7, stride 2, pad 3,
 * no bias) + bn1 (eval, folded by the host) + ReLU, reading the boundary NCHW bbox mask [n_src, 1, in_h, in_w] and writing NHWC
 * [n_img, in_h/2, in_w/2, out_cs].  w_pre: float[9][3] (tap-major), w7: float[49][3][64] (tap, cin, cout) with the BN scale
 * folded in, bias[64].  n_src / n_valid as in i2r_stem_conv (mirrored copies for the flip test, capacity padding). */
I2R_API int i2r_pe_res_stem(const float* mask_nchw, const float* w_pre, const float* w7, const float* bias, float* out_nhwc,
                    int32_t n_img, int32_t in_h, int32_t in_w, int32_t cout, int32_t out_cs, int32_t n_src, int32_t n_valid, void* stream);

/* i2r_pe_cat_vec -- PositionEmbeddingImage mode 'cat_vec' (position_embedding.py:19-23,69-87): per person, the boundary NCHW bbox mask
 * [n_src, 1, in_h, in_w] max-pooled `rate` times (MaxPool2d(3, 2, 1)) down to th x tw, flattened, through nn.Linear(th*tw, vec)
 * (w: float[vec][th*tw] as the reference stores it, bias[vec]), the resulting vector repeated over the th*tw tokens of the person:
 * written into channels [c0, c0 + vec) of the NHWC token rows out [n_img, th, tw, out_cs]; channels [c0 + vec, c_end) get zeros.
 * c0 = 0: the additive embedding of interformer_pureMulti.py:757,770 / interformer_2stage.py:398-406 (vec = DIM_MODEL there);
 * c0 = DIM_MODEL: the second half of torch.cat([x, multi_pos], dim=2) in interformer.py:296-298 (the first half is written by
 * the launch that produces x).  n_src / n_valid as in i2r_stem_conv (mirrored copies for the flip test, capacity padding). */
typedef struct i2r_pe_cat_vec_args {
    const float* in; const float* w; const float* bias; float* out;
    int32_t n_img, in_h, in_w, th, tw, rate, vec, out_cs, c0, c_end, n_src, n_valid;
} i2r_pe_cat_vec_args;
I2R_API int i2r_pe_cat_vec(const i2r_pe_cat_vec_args* a, void* stream);

/* i2r_maxpool3x3s2 -- nn.MaxPool2d(kernel_size=3, stride=2, padding=1) on NHWC
 * (interformer.py:162,260-264; position_embedding.py:9,106-109).  c % 4 == 0. */
I2R_API int i2r_maxpool3x3s2(const float* in, float* out, int32_t n_img, int32_t in_h, int32_t in_w, int32_t c,
                     int32_t in_cs, int32_t out_cs, void* stream);

/* i2r_head -- final 1x1 conv (with bias) NHWC -> boundary NCHW heatmaps
 * (final_layer, interformer_pureMulti.py:486-492,776; interformer.py:176-182,317).
 * w: float[cout][cin] (the nn.Conv2d weight as is), bias[cout]. out: [n_img, cout, h, w].
 * cin % 4 == 0, 1 <= cout <= 32.  cin a multiple of 16 up to 128 runs on the matrix pipe; any other cin keeps its weights
 * in 64 KB of LDS: cin <= 1024 (cout <= 16), 816 (cout <= 20), 512 (cout <= 32), beyond that I2R_E_ARG and no launch. */
I2R_API int i2r_head(const float* in, const float* w, const float* bias, float* out_nchw, int32_t n_img, int32_t h,
             int32_t w_, int32_t cin, int32_t in_cs, int32_t cout, void* stream);

/* i2r_conv_kernel_name -- which instantiation conv_igemm_f32<MT, NT, CAP, PF> a (grouped) launch resolves to, as it
 * appears in rocprofv3 kernel traces (used by bench.py to key its per-kernel roofline numbers). No launch happens. */
I2R_API int i2r_conv_kernel_name(const i2r_conv_desc* const* descs, int32_t n, char* buf, int32_t buflen);

/* i2r_conv_grid -- the workgroup count of a (grouped) launch as i2r_conv_grouped would issue it, with (with_map != 0: the length its
 * block_map must have) or without a dispatch table, and the run length it resolves for each member (seq: int32[n], may be null; 1 for
 * everything but algo 1).  No launch happens. */
I2R_API int i2r_conv_grid(const i2r_conv_desc* const* descs, int32_t n, int32_t with_map, int32_t* grid, int32_t* seq);

/* i2r_conv_wino_form -- the epilogue form an algo 1 (grouped) launch resolves to (additive: I2R_ABI_VERSION unchanged): 1 = bias + ReLU,
 * 2 = bias + res1 + ReLU -- every member has relu, no res2 / res_post, cout == cout_pad <= out_cs, and the members agree on res1 -- compiled
 * without flag tests; 0 = the general epilogue (everything else, other algorithms, and every launch while the forms are switched off).
 * The results do not depend on the form, bit for bit; kernel names (i2r_conv_kernel_name) do not report it.  No launch happens. */
I2R_API int i2r_conv_wino_form(const i2r_conv_desc* const* descs, int32_t n, int32_t* form);
/* i2r_conv_wino_forms -- process-wide switch (atomic): on != 0 (the default) lets algo 1 launches take the forms 1 / 2, 0 makes every
 * launch run the general epilogue.  Always I2R_OK. */
I2R_API int i2r_conv_wino_forms(int32_t on);

/* i2r_conv_direct_form -- what an fp32 algo 0 (grouped) launch of a double-buffered variant (conv_igemm_f32<MT, NT, CAP, PF> with PF > 0)
 * resolves to (additive: I2R_ABI_VERSION unchanged).  *form: 1 = every member has one channel chunk (the single-chunk body), 2 = the
 * pipelined body, 0 = the general body (PF 0, 16-bit operands, algo 1, and every launch while the forms are switched off).  *epi (may be
 * null): the epilogue form under the rule of i2r_conv_wino_form plus rep == 1 -- 1 = bias + ReLU, 2 = bias + res1 + ReLU, 0 = the general
 * epilogue (always 0 with form 0).  The results do not depend on either, bit for bit; kernel names do not report them.  No launch happens. */
I2R_API int i2r_conv_direct_form(const i2r_conv_desc* const* descs, int32_t n, int32_t* form, int32_t* epi);
/* i2r_conv_direct_forms -- process-wide switch (atomic): on != 0 (the default) lets such launches take the forms, 0 makes every launch
 * run the general body and epilogue.  Always I2R_OK. */
I2R_API int i2r_conv_direct_forms(int32_t on);

/* ---- after the forward: flip-test merge and keypoint decode -------------------------------- */
/* i2r_flip_merge -- out = (y + flip_back(y_flipped)) * 0.5  with flip_back = reverse W + swap left/right joints
 * (lib/core/function.py:142-162, lib/utils/transforms.py:16-30). joint_map: device int32[joints], the joint whose mirrored
 * heatmap lands in channel j (identity for unpaired joints). NCHW fp32 [n, joints, h, w].  Every element reads only its own y, so
 * out may be y itself (not y_flipped).  n == 0 returns I2R_OK without a launch and writes nothing.  n < 0, joints < 1, h < 1, w < 1,
 * more than 2^31 - 1 workgroups of 256 elements: I2R_E_ARG. */
I2R_API int i2r_flip_merge(const float* y, const float* y_flipped, const int32_t* joint_map, float* out, int32_t n, int32_t joints,
                   int32_t h, int32_t w, void* stream);

/* i2r_decode -- get_final_preds (lib/core/inference.py:90-112): arg-max (:20-48), Gaussian blur with kernel TEST.BLUR_KERNEL
 * on a zero-bordered copy re-normalised to the original max (:73-87), log(max(.,1e-10)), second-order Taylor refinement (:51-70),
 * inverse crop affine with rot 0 (lib/utils/transforms.py:50-101: scale about the centres by (scale[0]*200-1)/(w-1)).
 * The blur filters with the coefficients of cv2.GaussianBlur(dr, (k, k), 0), i.e. of getGaussianKernel(k, sigma <= 0): for k = 1, 3,
 * 5, 7 OpenCV's fixed table (small_gaussian_tab, modules/imgproc/src/smooth.dispatch.cpp: {1}, {.25, .5, .25}, {.0625, .25, .375,
 * .25, .0625}, {.03125, .109375, .21875, .28125, .21875, .109375, .03125}), from k = 9 on the Gaussian with sigma =
 * 0.3*((k-1)*0.5-1)+0.8 normalised to sum 1.  Both are restated from the OpenCV source; parity with cv2 rests on that source and has
 * not been run against cv2.  blur_kernel: odd, 1..31.  blur_kernel == 1 cannot run in the reference at all (its dr[0:-0] is empty);
 * here it is accepted and defined as "no blur".
 * heatmaps [n, joints, h, w]; center, scale [n, 2] (unused when transform_back == 0); preds [n, joints, 2]; maxvals [n, joints].
 * One workgroup per map with 2*h*w floats of LDS: h*w <= 19200 (150 KB; 160 x 120).  n == 0 returns I2R_OK without a launch and
 * writes nothing.  n < 0, joints < 1, h < 1, w < 2, n*joints beyond 2^31 - 1, a map above the LDS limit: I2R_E_ARG. */
I2R_API int i2r_decode(const float* heatmaps, const float* center, const float* scale, float* preds, float* maxvals, int32_t n,
               int32_t joints, int32_t h, int32_t w, int32_t blur_kernel, int32_t transform_back, void* stream);

/* i2r_joint_tokens -- heat maps to the query tables of i2r_attn_query_maps, on the device (additive: I2R_ABI_VERSION unchanged): the
 * literal get_max_preds (lib/core/inference.py:20-48) of every map, with the arg-max of i2r_decode (first index wins a tie; a map whose
 * maximum is not > 0 gives the point (0, 0): pred_mask), scaled to the crop's network input and mapped onto the token map of up to
 * I2R_MAX_TOKEN_TABLES encoder stacks the way visualize.py:194-196 does.  With (px, py) the arg-max pixel of map (s, j):
 *   points[s, j]  = (px * in_stride, py * in_stride)    fp32 [n_crops, joints, 2], optional (NULL)
 *   maxvals[s, j] = the map's maximum                   fp32 [n_crops, joints],    optional (NULL)
 *   table t:  tokens[crop_group[s] * K + crop_slot[s] * joints + j] = crop_slot[s] * fh * fw + row * fw + col,
 *             row = min(py * in_stride / down, fh - 1), col = min(px * in_stride / down, fw - 1)   (integer division)
 *   heatmaps  device fp32 [n_crops, joints, hh, hw] (NCHW, dense: what i2r_head and i2r_flip_merge write); in_stride: input pixels
 *             per heat-map pixel
 *   tokens    device int32 [n_grp, K], K >= joints the row stride: the q_tok of the stack's i2r_attn_query_maps launches.  The WHOLE
 *             table is set to -1 (a skipped entry) ahead of the kernel, so every entry no crop writes reads -1 afterwards
 *   crop_group, crop_slot  device int32 [n_crops]: the group of crop s in that stack and its place among the group's persons (an
 *             intra-human stack: (s, 0); the inter-human stack: (image, person)).  The host entry point cannot check a device
 *             table: the kernel skips the write of a crop whose group is outside [0, n_grp) or whose slot is negative or does not
 *             fit the row ((slot + 1) * joints > K) -- it forms no address from an entry it has not checked
 *   fh, fw, down  the stack's token map and its down rate (input pixels per token)
 * One wave per map, a 64-lane butterfly, no LDS, no atomics, vector stores only: deterministic.  n_tables == 0 writes points / maxvals
 * only.  I2R_E_ARG (nothing is launched or set): null a / heatmaps / table pointers, no output at all, n_crops, joints, hh, hw or
 * in_stride < 1, hh * hw or max(hh, hw) * in_stride beyond 2^31 - 1, n_tables outside 0 .. 2, a table with n_grp, fh, fw or down < 1,
 * K < joints or n_grp * K or (K / joints) * fh * fw beyond 2^31 - 1, n_crops * joints beyond 2^31 - 1 (the grid). */
#define I2R_MAX_TOKEN_TABLES 2
typedef struct i2r_token_table { int32_t* tokens; const int32_t* crop_group; const int32_t* crop_slot; int32_t n_grp, K, fh, fw, down, reserved; } i2r_token_table;
typedef struct i2r_joint_tokens_args {
    const float* heatmaps; float* points; float* maxvals; i2r_token_table table[I2R_MAX_TOKEN_TABLES /* 2 */];
    int32_t n_crops, joints, hh, hw, in_stride, n_tables;
} i2r_joint_tokens_args;
I2R_API int i2r_joint_tokens(const i2r_joint_tokens_args* a, void* stream);

/* i2r_pose_nms -- what every dataset class of the reference does with the decoded key points before it writes a result: the per-person
 * rescoring (lib/dataset/coco.py:384-396, same block in crowdpose.py / ochuman.py / coco_ochuman.py) and the per-image OKS-NMS or
 * soft-OKS-NMS (lib/nms/nms.py:75-181).  One workgroup per image.
 *   rescoring  score = mean of maxvals[j] over the joints with maxvals[j] > in_vis_thre (0 if none) * box_score; fp32, joints added in
 *              ascending order, one division, one multiplication: bit-identical to the reference's float32 value
 *   OKS        e_j = (dx^2 + dy^2) / (2 sigma_j)^2 / ((area_g + area_d) / 2 + spacing(1)) / 2, oks = mean_j exp(-e_j); dx^2 + dy^2 in fp32
 *              (the reference's key points are float32), the rest in fp64.  use_oks_vis != 0: only the joints of the CANDIDATE d with
 *              maxvals > oks_vis_thre count (nms.py:95 evaluates to that mask alone); no such joint: oks = 0.  The dataset classes
 *              never pass that threshold: use_oks_vis = 0 is the reference's evaluate()
 *   hard form  descending score; keep the head, drop every remaining person with oks(head, person) > oks_thre, repeat (max_dets unused)
 *   soft form  (soft = 1) take the head, multiply every remaining score by exp(-oks^2 / oks_thre), re-sort, stop after max_dets (20 in
 *              the reference; <= 0: no limit).  The decayed scores stay inside the kernel: `score` is the rescored value
 *   equal scores: the person with the lower crop index first (the reference's order is that of an unstable sort: undefined)
 * Inputs (device): preds [n_crops, joints, 2] and maxvals [n_crops, joints] as i2r_decode writes them; area [n_crops], or, when area is
 * null, scale [n_crops, 2] with area = (scale_x * 200) * (scale_y * 200) in fp32 (lib/core/function.py:220); box_score [n_crops];
 * img_off int32 [n_img + 1]: crop offset of every image (prefix sums of `length`, img_off[n_img] <= n_crops); sigmas [joints].
 * max_persons: HOST-side upper bound of the persons of one image (sizes the LDS; 1..1024, more is I2R_E_ARG and nothing is launched).
 * Outputs (device, per crop / per image, fixed size): score [n_crops] fp32; rank int32 [n_crops]: position in the reference's `keep`
 * list of the crop's image, -1 = suppressed or cut by max_dets; n_keep int32 [n_img].  An image whose offsets do not describe the
 * batch (negative count, beyond n_crops, more than max_persons persons) gets n_keep = -1 and nothing else written.  Crops outside
 * [img_off[0], img_off[n_img]) are not written.  n_crops == 0 or n_img == 0 returns I2R_OK at once.  1 <= joints <= 32. */
typedef struct i2r_pose_nms_args {
    const float* preds; const float* maxvals; const float* scale; const float* area; const float* box_score;
    const int32_t* img_off; const float* sigmas;
    float* score; int32_t* rank; int32_t* n_keep;
    double in_vis_thre, oks_thre, oks_vis_thre;
    int32_t n_crops, n_img, joints, max_persons, soft, max_dets, use_oks_vis, reserved;
} i2r_pose_nms_args;
I2R_API int i2r_pose_nms(const i2r_pose_nms_args* a, void* stream);

/* i2r_group_nearest -- the person groups of the reference's grouped test mode (PATCH_MODE main_target, lib/dataset/collater.py:28-51,
 * 164-173).  Per image of n persons and p = max_patch: n == 1 gives one group [0]; otherwise every person t ("target") gets a group of
 * k = min(n, p) members: t first, then the k - 1 other persons of the image smallest by the key (d(t, j), j), with
 * d = (ax_t - ax_j)^2 + (ay_t - ay_j)^2 in float64, every operation rounded on its own.  That is the reference's order (np.linalg.norm
 * of the anchor difference, a stable sort by it) whenever nobody else shares the target's anchor; with shared anchors the reference may
 * put another person first, here the target always is.  One wave per target, no atomics: deterministic.
 *   anchors     float64 [n_persons, 2] (device): the boxes' top-left corners (box[0], box[1])
 *   person_off  int32 [n_img + 1] (device): the images' first persons; person_off[n_img] = n_persons
 *   member_off  int32 [n_img + 1] (device): the images' first slots in `members`: member_off[b + 1] - member_off[b] = 1 for n = 1, else
 *               n * min(n, p) -- known on the host from the person counts alone; member_off[n_img] = n_members
 *   members     int32 [n_members] (device): global person indices, group after group (group g of the call is person g's).  A slot nobody
 *               qualifies for (non-finite anchors) holds -1.  Nothing outside [0, n_members) and nothing outside an image's own slot
 *               range is written; an image whose offsets do not describe the batch is skipped.
 * max_patch outside 1..64, negative counts, n_members < n_persons: I2R_E_ARG.  n_persons == 0 or n_img == 0 returns I2R_OK without a
 * launch; otherwise a null pointer is I2R_E_ARG. */
I2R_API int i2r_group_nearest(const double* anchors, const int32_t* person_off, const int32_t* member_off, int32_t n_img, int32_t n_persons,
                              int32_t n_members, int32_t max_patch, int32_t* members, void* stream);

/* ---- keypoint OKS evaluation: what COCOeval(gt, dt, 'keypoints') computes from the rows above (pycocotools cocoeval.py; the package is
 * not part of this project, so parity with its output is unpinned: the yardstick is the float64 restatement tests/_cocoeval_ref.py) ----
 * i2r_oks_match -- computeOks + evaluateImg of every image, every area range and every threshold.  One workgroup per image.
 * Detections are fp32 (as i2r_decode / i2r_pose_nms write them; the conversion to double is exact), everything else is float64 and
 * all arithmetic is fp64 without contraction, no floating-point atomics: two runs give the same bits.
 *   order      per image by descending score, equal scores: the lower index first (pycocotools' mergesort on -score; a NaN score ranks
 *              as -inf); only the first max_dets take part.  dt_valid (optional): a zero entry means the detection does not exist
 *   det. area  (max x - min x) * (max y - min y) over its J points (loadRes, key-point branch)
 *   OKS(d, g)  var_j = (2 sigma_j)^2, k1 = #{v_j > 0}.  k1 > 0: dx = xd - xg, dy = yd - yg.  k1 == 0: with the bbox (x, y, w, h),
 *              x0 = x - w, x1 = x + 2 w, y0 = y - h, y1 = y + 2 h, dx = max(0, x0 - xd) + max(0, xd - x1), dy likewise.
 *              e_j = (dx^2 + dy^2) / var_j / (area_g + 2^-52) / 2;  oks = sum of exp(-e_j) over the joints with v_j > 0 (k1 > 0) or over
 *              all J (k1 == 0), joints in ascending order, divided by their number
 *   gtIg       for area range a: gtIg[g] = ignore_g or area_g < lo_a or area_g > hi_a (bounds inclusive); the gts are walked
 *              non-ignored first, each class in input order (a stable sort)
 *   matching   for each threshold t, detections in score order: iou = min(t, 1 - 1e-10), m = -1; over the gts in walk order: skip a gt
 *              already matched at t unless it is a crowd; BREAK when m is a non-ignored gt and this gt is ignored; skip when oks < iou;
 *              else iou = oks, m = g.  A match marks the gt and gives the detection dtIg = gtIg[m]; an unmatched detection is ignored
 *              when its own area lies outside [lo_a, hi_a]
 * Inputs (device): dt_kpts fp32 [n_dt, joints, 2]; dt_score fp32 [n_dt]; dt_valid uint8 [n_dt] or null; dt_off int32 [n_img + 1]
 * (detections grouped by image); gt_kpts f64 [n_gt, joints, 3] (x, y, v); gt_area f64 [n_gt]; gt_bbox f64 [n_gt, 4] (x, y, w, h);
 * gt_flags int32 [n_gt]: bit 0 = iscrowd, bit 1 = ignore (= iscrowd or num_keypoints == 0, computed by the host); gt_off int32
 * [n_img + 1]; sigmas f64 [joints]; thr f64 [n_thr], 1 <= n_thr <= 16; area_rng f64 [n_area, 2], 1 <= n_area <= 4.
 * max_dets 1..32; max_dt_per_img (0..1024) and max_gt_per_img (0..256): HOST-side upper bounds of one image's counts (they size the
 * LDS); 1 <= joints <= 32.  Anything beyond these: I2R_E_ARG and nothing is launched.
 * Outputs (device, fixed size): dt_rank int32 [n_dt]: position in the image's score order, -1 = not valid or beyond max_dets;
 * dt_match, dt_ignore uint32 [n_area, n_dt]: bit t = threshold t (0 for a detection of rank -1); gt_ignore uint8 [n_area, n_gt];
 * oks (optional) f64 with oks_off int64 [n_img + 1] and oks_len, the element count of the buffer: the [D, G] matrix of image i lies
 * row-major in INPUT order at oks_off[i]; rows of detections of rank -1 hold -1.0; an image whose matrix would not lie inside
 * [0, oks_len) gets none.  Nothing outside [dt_off[0], dt_off[n_img]) / [gt_off[0], gt_off[n_img]) is written.  An image whose offsets
 * do not describe the batch (negative count, beyond n_dt / n_gt, more than the host-side bounds) gets rank -1 for those of its own
 * detections that lie inside [0, n_dt) and nothing else.  n_img == 0 returns I2R_OK without a launch. */
typedef struct i2r_oks_match_args {
    const float* dt_kpts; const float* dt_score; const uint8_t* dt_valid; const int32_t* dt_off;
    const double* gt_kpts; const double* gt_area; const double* gt_bbox; const int32_t* gt_flags; const int32_t* gt_off;
    const double* sigmas; const double* thr; const double* area_rng;
    int32_t* dt_rank; uint32_t* dt_match; uint32_t* dt_ignore; uint8_t* gt_ignore; double* oks; const int64_t* oks_off;
    int64_t oks_len;
    int32_t n_dt, n_gt, n_img, joints, n_thr, n_area, max_dets, max_dt_per_img, max_gt_per_img, reserved;
} i2r_oks_match_args;
I2R_API int i2r_oks_match(const i2r_oks_match_args* a, void* stream);

/* i2r_oks_accumulate -- COCOeval.accumulate for one category and one maxDets.  One workgroup per (group, area range, threshold); group
 * index n_group is "every image", whatever img_group says.  Per (group, a, t):
 *   npig = number of gts with gtIg == 0 in the group's images; npig == 0: precision and recall stay -1
 *   tp, fp = cumulative counts of (match and not ignore), (not match and not ignore) along `order`, restricted to the group's images
 *   rc = tp / npig, pr = tp / ((fp + tp) + 2^-52); recall = the last rc, 0 without detections; pr made non-increasing from the back;
 *   precision[r] = pr[first i with rc[i] >= rec_thr[r]], 0 when there is none
 * The counts are integers and every division is one fp64 division of exact operands: precision and recall equal numpy's bit for bit.
 * The walk is a block-wide scan over chunks of 1024 entries from the back with a running maximum; the cumulative counts at a chunk's
 * start are the totals of a first counting pass minus what lies behind, so the kernel needs NO workspace.
 * Inputs (device): dt_match, dt_ignore [n_area, n_dt] and gt_ignore [n_area, n_gt] as i2r_oks_match writes them; dt_rank [n_dt] or
 * null; order int32 [n_part]: detections in global stable descending-score order, the images in ascending order and inside an image
 * the rank order as the pre-sort order (entries outside [0, n_dt), and entries whose dt_rank is negative, take no part); dt_img int32
 * [n_dt]: image index of a detection; img_group int32 [n_img]: group of an image, -1 = in none (null when n_group == 0); gt_off int32
 * [n_img + 1]; rec_thr f64 [n_rec], 1 <= n_rec <= 128.  1 <= n_thr <= 16, 1 <= n_area <= 4, n_group >= 0.
 * Outputs (device): precision f64 [n_group + 1, n_thr, n_rec, n_area]; recall f64 [n_group + 1, n_thr, n_area]; npig int32
 * [n_group + 1, n_area].  All of them are written by every call (n_part == 0 included). */
typedef struct i2r_oks_accumulate_args {
    const uint32_t* dt_match; const uint32_t* dt_ignore; const int32_t* dt_rank; const int32_t* order; const int32_t* dt_img;
    const int32_t* img_group; const uint8_t* gt_ignore; const int32_t* gt_off; const double* rec_thr;
    double* precision; double* recall; int32_t* npig;
    int32_t n_dt, n_gt, n_img, n_part, n_group, n_thr, n_area, n_rec;
} i2r_oks_accumulate_args;
I2R_API int i2r_oks_accumulate(const i2r_oks_accumulate_args* a, void* stream);

/* ---- the two numbers validate() logs per batch: loss and PCK accuracy (lib/core/function.py:167-174) ------------------------------
 * i2r_joint_targets -- JointsDataset.generate_target + adjust_target_weight (lib/dataset/JointsDataset.py:394-450), target_type
 * 'gaussian', for every (crop, joint).  One workgroup per map.
 *   weight     target_weight = joints_vis; tmp_size = 3 * sigma, ul = int(mu - tmp_size), br = int(mu + tmp_size + 1) with int()
 *              truncating toward zero (so br < 0 means mu + tmp_size + 1 <= -1); weight -> 0 when ul_x >= w or ul_y >= h or br_x < 0 or
 *              br_y < 0
 *   map        exp(-((x - mu_x)^2 + (y - mu_y)^2) / (2 sigma^2)) over the WHOLE map (this reference has no 13 x 13 window), drawn only
 *              when the adjusted weight is > 0.5; otherwise the map is zero while a non-zero weight still reaches the loss.  The
 *              argument is evaluated in fp64 as the reference does (no contraction), rounded to fp32, one expf: within 2.5e-7 of the reference's value
 *   joints_weight (optional, LOSS.USE_DIFFERENT_JOINTS_WEIGHT) multiplies the weight AFTER that decision, in fp32
 * Inputs (device): joints_hm float64 [n_crops, joints, 2], (x, y) in heat-map pixels -- float64 because the reference's joints_3d is
 * (an fp32 mu of 50 px is off by 4e-6 px, which alone moves map values by 6e-7); joints_vis fp32 [n_crops, joints] (column 0 of the
 * reference's array); joints_weight fp32 [joints] or null.  sigma > 0 (MODEL.SIGMA).
 * Outputs (device): target_weight fp32 [n_crops, joints]; target fp32 [n_crops, joints, h, w], or null: only the weights are written.
 * n_crops == 0 returns I2R_OK without a launch.  joints < 1, h < 1, w < 1, n_crops * joints or h * w beyond 2^31 - 1: I2R_E_ARG. */
typedef struct i2r_joint_targets_args {
    const double* joints_hm; const float* joints_vis; const float* joints_weight;
    float* target_weight; float* target;
    double sigma;
    int32_t n_crops, joints, h, w;
} i2r_joint_targets_args;
I2R_API int i2r_joint_targets(const i2r_joint_targets_args* a, void* stream);

/* i2r_val_metrics -- JointsMSELoss.forward (lib/core/loss.py:15-41) + accuracy (lib/core/evaluate.py:16-71, get_max_preds
 * lib/core/inference.py:20-48) in one pass over the prediction `output` fp32 [n_crops, joints, h, w].  Two launches: one workgroup per
 * map, then one workgroup that adds the per-map partials up in a fixed order (no floating-point atomics: two runs give the same bits).
 * The target comes in ONE of two forms (both or neither: I2R_E_ARG):
 *   tensor    target fp32 [n_crops, joints, h, w] + target_weight fp32 [n_crops, joints] (may be null when use_target_weight == 0)
 *   analytic  joints_hm, joints_vis, joints_weight, sigma as i2r_joint_targets takes them (target and target_weight null): every target
 *             value is evaluated in the kernel, never stored or read
 * Per map:
 *   sum of (p * w - t * w)^2, every one of the four fp32 operations rounded on its own as torch does them, accumulated in fp64;
 *             use_target_weight == 0: (p - t)^2
 *   arg-max   first flat index of the maximum of p, and of t; coordinates (idx % w, floor(idx / w)), both 0 when the maximum is not > 0
 * Results (device, all required but meter):
 *   sse float64 [joints] raw sums; loss float64 [1] = sum_j 0.5 * sse[j] / (n_crops * h * w) / joints
 *   hits, valid int32 [joints]; acc float64 [joints + 1]; avg_acc float64 [1]; cnt int32 [1] -- accuracy / calc_dists / dist_acc:
 *             a (crop, joint) counts only when the TARGET's arg-max has x > 1 and y > 1; norm = [h, w] / 10 meets (x, y) in that order
 *             (x is divided by h / 10); dist = sqrt((px / n0 - tx / n0)^2 + (py / n1 - ty / n1)^2) in fp64, divided THEN subtracted; a hit
 *             is dist < 0.5; acc[j + 1] = hits[j] / valid[j], or -1 when no crop counts, which keeps the joint out of avg_acc (the mean
 *             of the others) and cnt; acc[0] = avg_acc (0 when cnt == 0)
 *   pred fp32 [n_crops, joints, 2]: the arg-max coordinates of the prediction (accuracy's fourth return value)
 *   meter (optional) float64 [4], caller-owned and caller-zeroed: += loss * n_crops, n_crops, avg_acc * cnt, cnt in stream order -- the
 *             sums and counts of validate()'s two AverageMeters
 * sse, hits and valid are raw so that shards of a data-parallel step can be combined exactly: i2r_val_combine below takes the rows
 * (n_crops, sse, hits, valid) of several parts and applies this entry's own finishing step to their totals.
 * ws: workspace of 16 * n_crops * joints bytes, 8-byte aligned, contents irrelevant before and after.
 * n_crops == 0 returns I2R_OK without a launch and writes nothing.  joints < 1, h < 1, w < 1, counts beyond 2^31 - 1: I2R_E_ARG. */
typedef struct i2r_val_metrics_args {
    const float* output;
    const float* target; const float* target_weight;                                  /* tensor form */
    const double* joints_hm; const float* joints_vis; const float* joints_weight;     /* analytic form */
    void* ws;
    double* loss; double* acc; double* avg_acc; int32_t* cnt; float* pred; double* sse; int32_t* hits; int32_t* valid; double* meter;
    double sigma;
    int32_t n_crops, joints, h, w, use_target_weight, reserved;
} i2r_val_metrics_args;
I2R_API int i2r_val_metrics(const i2r_val_metrics_args* a, void* stream);

/* i2r_val_combine -- the finishing step of i2r_val_metrics over the raw sums of several parts (the shards of a data-parallel step, one
 * row per rank as an all-gather stacks them): the loss, accuracy and meter update of the WHOLE batch, on every rank the same bits.
 * Input (device): parts float64 [n_part, 1 + 3 * joints]; row r = n_crops_r, sse_r[joints], hits_r[joints], valid_r[joints] -- the
 *   integers travel as doubles (exact below 2^53).  A part with n_crops <= 0 contributes nothing (a rank without images launches no
 *   i2r_val_metrics and hands in zeros).  h, w: the heat-map size the parts were computed at.
 * One launch of one workgroup, no workspace, no floating-point atomics: a thread owns joints j, j + blockDim, ... and adds the parts in
 * ascending part index, so two runs -- and two ranks -- give the same bits.  One thread then forms loss, acc, avg_acc, cnt and the meter
 * update with the expressions of i2r_val_metrics, in its order, with n_crops = the total: n_part == 1 reproduces i2r_val_metrics' own
 * loss, acc, avg_acc, cnt and meter bit for bit.
 * Results (device, all required but meter), shapes and meanings as i2r_val_metrics gives them:
 *   sse float64 [joints], hits, valid int32 [joints]: the totals; loss float64 [1]; acc float64 [joints + 1]; avg_acc float64 [1];
 *   cnt int32 [1]; n_crops int32 [1]: the total crop count S
 *   meter (optional) float64 [4]: += loss * S, S, avg_acc * cnt, cnt in stream order
 * hits, valid, acc, avg_acc, cnt and n_crops are exact; sse and loss are fp64 sums of non-negative terms in another order than one
 * i2r_val_metrics call over the whole batch uses: within (number of terms - 1) * 2^-53 relative of it.
 * Total crop count 0: every result is written as 0 (acc too), the meter is left alone, nothing is divided.
 * Precondition: the total crop count (and with it every total of hits and valid) is <= 2^31 - 1.
 * n_part < 1, joints < 1, h < 1, w < 1 or a null required pointer: I2R_E_ARG without a launch. */
typedef struct i2r_val_combine_args {
    const double* parts;
    double* sse; int32_t* hits; int32_t* valid;
    double* loss; double* acc; double* avg_acc; int32_t* cnt; int32_t* n_crops; double* meter;
    int32_t n_part, joints, h, w;
} i2r_val_combine_args;
I2R_API int i2r_val_combine(const i2r_val_combine_args* a, void* stream);

/* ---- head re-fit: the gradient of the validation loss with respect to final_layer, on frozen features ---------------------------
 * i2r_head_grad -- JointsMSELoss.forward (lib/core/loss.py:15-41) behind a 1x1 final_layer with bias, differentiated with respect to
 * that layer's weight and bias, in one pass over the layer's INPUT (additive: I2R_ABI_VERSION unchanged).  No heat map, target map or
 * gradient map is stored.  Write N = n_crops * h * w_, J = joints:
 *   o[s,j,p] = sum_c w[j,c] feat[s,p,c] + bias[j]             (the fp32 matrix pipe: an fmaf chain over c that starts at the bias)
 *   t, tw     what i2r_val_metrics uses in the same form -- tensor: target fp32 [n_crops, joints, h, w_] (NCHW) + target_weight fp32
 *             [n_crops, joints] (may be null when use_target_weight == 0); analytic: joints_hm, joints_vis, joints_weight, sigma as
 *             i2r_joint_targets takes them (the adjusted weight, the draw decision at > 0.5, joints_weight after it, the Gaussian's
 *             argument in fp64).  Both forms or neither: I2R_E_ARG
 *   sse[j]  = sum_{s,p} (tw o - tw t)^2, the four fp32 operations of a term rounded separately, added up in fp64;
 *             use_target_weight == 0: (o - t)^2
 *   loss    = sum_j 0.5 * sse[j] / N / J
 *   g[s,j,p]= tw[s,j]^2 (o - t); use_target_weight == 0: o - t
 *   dw[j,c] = (sum_{s,p} g feat[s,p,c]) / (N J);  db[j] = (sum_{s,p} g) / (N J)
 * Inputs (device): feat fp32 NHWC, [n_crops, h, w_] rows of in_cs floats of which channels [0, cin) are read; w fp32 [joints] rows of
 * w_cs floats (the nn.Conv2d weight as is when w_cs == cin); bias fp32 [joints].
 * Results (device, all required): dw fp32 [joints][cin] dense, db fp32 [joints], loss float64 [1], sse float64 [joints].
 * Two launches.  Tile: one wave owns a run of 16-pixel fragments of ONE crop, runs both products on the fp32 matrix pipe and writes its
 * partial dw (fp32), db and sse (fp64) to the workspace.  Finish: every output is the fp64 sum of its partials in a fixed order, divided
 * once by N J in fp64 and rounded once to fp32.  No floating-point atomics: two runs give the same bits, whatever the workspace held.
 * No fp32 accumulator ever sums more than one crop's pixels: with u = 2^-24 the result is within
 *   ((cin + 1) u (sum_c |w||f| + |b|) tw^2 + 4 u |g|) per gradient element (+ 2.5e-7 tw^2 for a drawn analytic target), and
 *   (h w_ + 4) u sum |g||f| / (N J) + u |dw| on top for the sums, of the same expressions evaluated in float64.
 * ws: workspace of i2r_head_grad_ws_bytes bytes, 8-byte aligned, contents irrelevant before and after.
 * Limits: 1 <= joints <= 32; cin a multiple of 16 in [16, 128] (the matrix-pipe range of i2r_head), cin <= in_cs, cin <= w_cs; feat
 * 16-byte aligned, in_cs % 4 == 0; h, w_ >= 1.  A violation returns I2R_E_ARG without a launch.  n_crops == 0 returns I2R_OK, launches
 * nothing and writes nothing. */
typedef struct i2r_head_grad_args {
    const float* feat;
    const float* w; const float* bias;
    const float* target; const float* target_weight;                                  /* tensor form */
    const double* joints_hm; const float* joints_vis; const float* joints_weight;     /* analytic form */
    void* ws;
    float* dw; float* db;
    double* loss; double* sse;
    double sigma;
    int32_t n_crops, h, w_, cin, in_cs, w_cs, joints, use_target_weight;
} i2r_head_grad_args;
I2R_API int i2r_head_grad(const i2r_head_grad_args* a, void* stream);
/* *bytes = the workspace size i2r_head_grad needs for this shape (a function of the shape alone; 0 for n_crops == 0).  A shape outside
 * the limits above, or a null bytes: I2R_E_ARG.  (A status return like every entry of this header; the size comes back through bytes.) */
I2R_API int i2r_head_grad_ws_bytes(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t* bytes);

/* i2r_head_normal -- the same fit in closed form.  With the features frozen JointsMSELoss is a quadratic in (W, b), separately per joint;
 * this entry collects its normal equations in one pass over the features (additive: I2R_ABI_VERSION unchanged).  Write
 * f~[s,p,:] = (feat[s,p,0..cin_out-1], 1), and take t and tw exactly as i2r_head_grad takes them (tensor or analytic form,
 * use_target_weight == 0: tw = 1).  The state is float64, on the device, in/out:
 *   A[j,a,b] += sum_s tw[s,j]^2 sum_p f~[s,p,a] f~[s,p,b]      [joints][cin_out + 1][cin_out + 1], symmetric, stored whole
 *   r[j,a]   += sum_s tw[s,j]^2 sum_p f~[s,p,a] t[s,j,p]       [joints][cin_out + 1]
 *   c[j]     += sum_s sum_p (tw[s,j] t[s,j,p])^2               [joints]   (what i2r_head_grad's sse[j] is at w = 0, bias = 0)
 *   n        += n_crops * h * w_                               int64 [1]
 * Over everything accumulated the loss of a head is L(W, b) = (1 / (2 n J)) sum_j (w~_j^T A_j w~_j - 2 w~_j^T r_j + c_j), w~_j =
 * (W[j,:], b[j]): JointsMSELoss of the concatenation of all batches added; its minimiser solves A_j w~_j = r_j per joint.
 * Rows of A and r are ld doubles apart (A[j][a][b] at (j * ld + a) * ld + b, r[j][a] at j * ld + a; ld > cin_out); what lies behind
 * cin_out + 1 in a row, and rows behind it, are not touched.  cin is the channel count the pass runs at (a multiple of 16); cin_out <=
 * cin is the true one: channels [cin_out, cin) are the caller's zero padding and get no state, the bias entry sits at index cin_out.
 * Two launches.  Tile: a workgroup of four waves owns a run of 16-pixel fragments of ONE crop, reads the features once, forms the
 * crop's Gram tiles (16-channel blocks ci <= cj only) on the fp32 matrix pipe, both operands being the read i2r_head_grad's second
 * product makes, the product (tw tw t)^T F the way i2r_head_grad forms dw, and the column sums F^T 1; it writes fp32 partials (fp64
 * for the sums that need no feature) to the workspace.  Finish: per crop the partials in ascending order in fp64, then weighted with
 * tw^2 (exact in fp64) across crops in a fixed order; every state element is updated by exactly one thread as state += sum.  No
 * floating-point atomics: equal state and inputs give equal bits, whatever the workspace held.  No fp32 accumulator ever sums more than
 * one crop's pixels: with u = 2^-24, k = h w_, against the same sums in float64
 *   |A - A*|[j,a,b] <= (k + 2) u sum_s tw^2 sum_p |f~_a||f~_b| + delta
 *   |r - r*|[j,a]   <= sum_s sum_p (tw^2 e_t + (k + 4) u |tw^2 t|) |f~_a| + delta   (e_t = 2.5e-7 for a drawn analytic target, else 0)
 *   c as i2r_head_grad's sse at o = 0; n exact; delta = (parts per crop + n_crops + 16) 2^-53 times the sum of absolute values (and
 *   one more rounding of the state the sum is added to).
 * ws: workspace of i2r_head_normal_ws_bytes bytes, 8-byte aligned, contents irrelevant before and after.
 * Limits: those of i2r_head_grad (1 <= joints <= 32; cin a multiple of 16 in [16, 128], cin <= in_cs; feat 16-byte aligned, in_cs % 4
 * == 0; h, w_ >= 1), 1 <= cin_out <= cin, ld > cin_out, state 8-byte aligned.  A violation returns I2R_E_ARG without a launch.
 * n_crops == 0 returns I2R_OK, launches nothing and touches nothing. */
typedef struct i2r_head_normal_args {
    const float* feat;
    const float* target; const float* target_weight;                                  /* tensor form */
    const double* joints_hm; const float* joints_vis; const float* joints_weight;     /* analytic form */
    void* ws;
    double* A; double* r; double* c; int64_t* n;
    double sigma;
    int32_t n_crops, h, w_, cin, in_cs, cin_out, ld, joints, use_target_weight, reserved;
} i2r_head_normal_args;
I2R_API int i2r_head_normal(const i2r_head_normal_args* a, void* stream);
/* *bytes = the workspace size i2r_head_normal needs for this shape (a function of the shape alone; 0 for n_crops == 0).  A shape outside
 * the limits above, or a null bytes: I2R_E_ARG. */
I2R_API int i2r_head_normal_ws_bytes(int32_t n_crops, int32_t h, int32_t w_, int32_t cin, int32_t joints, int64_t* bytes);

/* ---- input side (reference lib/dataset/JointsDataset.py:296-333) ------------------------
 * i2r_crop_affine -- cv2.warpAffine(image, trans, IMAGE_SIZE, INTER_LINEAR) + ToTensor + Normalize for the n persons of ONE
 * image: out[p][c][y][x] = (bilinear(img, M_p (x, y, 1)^T) / 255 - mean[c]) * inv_std[c], taps outside the image = 0.
 * img: device uint8 [ih, iw, 3] with row pitch row_bytes (HWC as cv2.imread delivers it; swap_rb = DATASET.COLOR_RGB);
 * inv_trans: device float [n, 6] = the INVERSE (input pixel -> image pixel) of get_affine_transform(center, scale, 0, size)
 * (lib/utils/transforms.py:61-96); out: [n, 3, oh, ow] fp32.  fp32 interpolation, NOT cv2's fixed-point one (parity unpinned:
 * cv2 is not available to pin it; deviation bounded by cv2's 1/32-pixel / 8-bit quantisation). */
I2R_API int i2r_crop_affine(const unsigned char* img, int32_t ih, int32_t iw, int32_t row_bytes, int32_t swap_rb, const float* inv_trans,
                    const float* mean, const float* inv_std, float* out, int32_t n, int32_t oh, int32_t ow, void* stream);

/* i2r_box_mask -- get_position(shape, box, 'single') + rotate_bound(., 0) + cv2.resize(., IMAGE_SIZE) + ToTensor
 * (JointsDataset.py:165-177,323-331): the filled inclusive rectangle boxes[p] = (int(x), int(y), int(x+w), int(y+h)) at image
 * resolution, resized bilinearly (half-pixel centres) to [n, 1, oh, ow], values in [0, 1].  Same parity note as above. */
I2R_API int i2r_box_mask(const int32_t* boxes, int32_t ih, int32_t iw, float* out, int32_t n, int32_t oh, int32_t ow, void* stream);

/* i2r_crop_affine_cv2 / i2r_box_mask_cv2 -- the same two steps in cv2's OWN arithmetic, restated from OpenCV's published algorithm
 * (imgwarp.cpp warpAffine -> remap with the 1/32-pixel fixed-point bilinear table, 15-bit weights, 8-bit result; resize.cpp 8-bit
 * linear resize with 11-bit coefficients; rotate_bound(mask, 0)'s half-pixel shift along odd image dimensions, JointsDataset.py:180-202).
 * inv_m: device double [n, 6] = the INVERSE of get_affine_transform(...) computed in double precision the way cv2.warpAffine does.
 * Default of the host side (input.person_inputs); still "parity unpinned": cv2 is absent from the build image, nothing could be
 * compared with a cv2 output (oracle/input_cpu.py carries the same restatement in numpy). */
I2R_API int i2r_crop_affine_cv2(const unsigned char* img, int32_t ih, int32_t iw, int32_t row_bytes, int32_t swap_rb, const double* inv_m,
                        const float* mean, const float* inv_std, float* out, int32_t n, int32_t oh, int32_t ow, void* stream);
I2R_API int i2r_box_mask_cv2(const int32_t* boxes, int32_t ih, int32_t iw, float* out, int32_t n, int32_t oh, int32_t ow, void* stream);

/* i2r_person_inputs_cv2 -- the input side of a whole validate() BATCH in one launch: for every person crop p of every image,
 * i2r_crop_affine_cv2 and i2r_box_mask_cv2 (same arithmetic, bit-identical results) written straight into the collated tensors
 * x_out [n_crops, 3, oh, ow] and mask_out [n_crops, 1, oh, ow] that collater.__call__ would build (lib/dataset/collater.py:14-26).
 * images / crops: DEVICE tables (the caller uploads both in one pinned, stream-ordered copy); crops[p].image indexes `images`;
 * the crops of an image must be consecutive for the model's `length` list to describe them, the kernel itself does not care.
 * The tables are device memory the host entry point cannot read: a crop whose `image` index lies outside [0, n_images) or whose
 * image entry is empty (null pointer, ih / iw <= 0) gets ZEROS in x_out / mask_out instead of an out-of-bounds read (the call
 * still returns I2R_OK); `reserved` fields are ignored.
 * mean / inv_std: HOST float[3] (passed on as kernel arguments). */
typedef struct {
    const unsigned char* img;      /* device uint8 [ih, iw, 3], channel order as cv2.imread delivers it */
    int32_t ih, iw, row_bytes, reserved;
} i2r_image_ref;                   /* 24 bytes */
typedef struct {
    double inv_m[6];               /* the INVERSE of get_affine_transform(center, scale, 0, size) in double, as cv2.warpAffine derives it */
    int32_t box[4];                /* (int(x), int(y), int(x + w), int(y + h)): the inclusive corners cv2.rectangle fills */
    int32_t image;                 /* index into the image table */
    int32_t reserved[3];
} i2r_crop_ref;                    /* 80 bytes */
I2R_API int i2r_person_inputs_cv2(const i2r_image_ref* images, int32_t n_images, const i2r_crop_ref* crops, int32_t n_crops, int32_t swap_rb,
                          const float* mean, const float* inv_std, float* x_out, float* mask_out, int32_t oh, int32_t ow, void* stream);

/* i2r_train_inputs_cv2 -- the TRAINING samples of a batch in one launch (additive: I2R_ABI_VERSION unchanged): what
 * JointsDataset.__getitem__ with is_train builds per person (lib/dataset/JointsDataset.py:233-334) -- the crop of the image, mirrored
 * where the draw flips it, under a map with rotation, rescaling and possibly the half-body box; and the person's box mask after
 * rotate_bound(mask, r) and cv2.resize -- written into the collated x_out [n_crops, 3, oh, ow] / mask_out [n_crops, 1, oh, ow] in
 * cv2's fixed-point arithmetic, as i2r_person_inputs_cv2 does for validation (same image table, same rules for mean / inv_std, same
 * parity note: restated from OpenCV's published algorithm, no cv2 output could be compared).
 *   crop   cv2.warpAffine(image[:, ::-1] if flip else image, trans, (ow, oh)): tap column xi of the mirrored image reads source column
 *          iw - 1 - xi, the border test is on xi; no second image is built.
 *   mask   the nW x nH canvas of rotate_bound is never built: an output pixel takes the 2 x 2 taps of cv2.resize from (nW, nH) to
 *          (ow, oh), each the fixed-point warpAffine (mask_inv_m) of the binary rectangle `box`, clipped to the image and mirrored with it.
 * A crop whose `image` index lies outside [0, n_images), whose image entry is empty (null pointer, ih / iw <= 0) or whose canvas is empty
 * (nw / nh <= 0) gets ZEROS in x_out / mask_out (the call still returns I2R_OK); `reserved` is ignored.  I2R_E_ARG without a launch: a
 * null pointer, n_images / n_crops / oh / ow <= 0, more than 2^31 - 1 workgroups of 256 output pixels. */
typedef struct {
    double inv_m[6];               /* the INVERSE of get_affine_transform(center, scale, rot, size) in double, as cv2.warpAffine derives it */
    double mask_inv_m[6];          /* the same inverse of rotate_bound's map: getRotationMatrix2D((iw / 2, ih / 2), rot, 1) + (nw / 2 - iw / 2, nh / 2 - ih / 2) */
    int32_t box[4];                /* (int(x), int(y), int(x + w), int(y + h)) of the UNFLIPPED image, clipped to it or not: the kernel clips */
    int32_t nw, nh;                /* rotate_bound's canvas: int(ih |sin| + iw |cos|), int(ih |cos| + iw |sin|) */
    int32_t image;                 /* index into the image table */
    int32_t flip;                  /* != 0: the sample is taken from the horizontally mirrored image */
    int32_t reserved[4];
} i2r_train_crop_ref;              /* 144 bytes */
I2R_API int i2r_train_inputs_cv2(const i2r_image_ref* images, int32_t n_images, const i2r_train_crop_ref* crops, int32_t n_crops, int32_t swap_rb,
                         const float* mean, const float* inv_std, float* x_out, float* mask_out, int32_t oh, int32_t ow, void* stream);

/* ---- HRFormer-B glue (reference lib/models/hrformer.py) ---------------------------------------------------- */
/* i2r_layernorm -- nn.LayerNorm(c, eps) over the channels of every pixel/token of an NHWC tensor
 * (GeneralTransformerBlock.norm1/norm2, hrformer.py:1198,1235-1237). w, b: [cs] zero-padded. */
I2R_API int i2r_layernorm(const float* in, const float* w, const float* b, float* out, int32_t npix, int32_t c, int32_t cs,
                  float eps, int32_t out_dt /* storage of out: 0 fp32, 1 bf16, 2 f16 */, void* stream);

/* i2r_window_attn -- the softmax(q k^T) v core of InterlacedPoolAttention / MHA_ over 7x7 windows
 * (hrformer.py:1164-1180, 692-935): centre zero-padding to multiples of 7 (:947-956), window gather (:978-987),
 * heads = c / head_dim, q scaled by head_dim^-0.5 (:780), NO relative-position bias (:883-885), de-pad (:958-964).
 * qkv: [n, h, w, 3*hs] holding the q | k | v projections of the LayerNorm-ed tokens (a 1x1 i2r_conv with the stacked
 * q/k/v_proj weights), each part hs = heads*40 wide: head hh's dim d at channel hh*40 + d, the pad channel(s) of a head
 * exactly zero (zero weight rows), q ALREADY scaled by head_dim^-0.5 (folded into q_proj by the host).
 * bias_qkv: [3*hs] = the projections of a zero token in the same layout (what padded tokens contribute).
 * out: [n, h, w, hs] attention output BEFORE out_proj, same head-padded channel order (out_proj gets zero columns there).
 * 36 < head_dim <= 40 (HRFormer-B: 39).  Runs on the fp32 matrix pipe: one workgroup per (crop, window, head). */
I2R_API int i2r_window_attn(const float* qkv, const float* bias_qkv, float* out, int32_t n_img, int32_t h, int32_t w, int32_t c,
                    int32_t hs, int32_t heads, void* stream);

/* i2r_hrt_attn_block -- 16-bit modes only: the attention half of a GeneralTransformerBlock in ONE launch,
 *     out = x + out_proj(window_attention(q|k|v_proj(LayerNorm(x))))      (hrformer.py:1230-1236; same semantics as
 * i2r_layernorm + i2r_conv(q|k|v) + i2r_window_attn + i2r_conv(out_proj, res1 = x)), one workgroup per 7x7 window, on
 * v_mfma_f32_16x16x32_{bf16,f16} with fp32 LayerNorm / softmax / accumulation; x and out are fp32 NHWC [n, h, w, cs] (may not alias).
 * Built for the four HRFormer-B branches: (c, heads, cs) = (78, 2, 80), (156, 4, 160), (312, 8, 320), (624, 16, 624); head_dim 39 padded
 * to 48.  variant: 0 = the library's choice; 1 = one wave per 16-token tile of the window, K / V^T through LDS (rounds 3-4; 78 / 156
 * only); 2 = one wave per HEAD over all 64 token rows, the whole attention of a head in registers, every weight fragment feeding four
 * matrix instructions (round 5; all four widths).  Same operands, same arithmetic, results agree to fp32 summation order.
 * Operand images (16-bit, fragment-packed for the 32-deep MFMA: element e of lane l of a fragment = M[16*rowblk + (l & 15)][32*kstep +
 * 8*(l >> 4) + e], 16 bytes per lane, 1 KB per fragment):
 *   wqkv  [head][q, k, v][cs/32 rounded up k-steps][3 dim blocks][64 lanes][8]: rows = the head's 39 output dims (+ 9 zero rows) of
 *         q_proj / k_proj / v_proj, columns = input channels (zero beyond cs); q rows (and bias) pre-multiplied by head_dim^-0.5 * log2(e);
 *   bqkv  float [head][3][48];
 *   wo    [cs/16 output blocks][heads*48/32 k-steps][64 lanes][8]: rows = out_proj outputs, columns = (head, dim) with zeros beyond 39,
 *         re-ordered inside every 32-column k-step to the kernel's slot order: slot 8g + 4h + r <- column 16 (2 kstep + h) + 4g + r
 *         (g < 4, h < 2, r < 4): the B operand of that GEMM is two 16-dim accumulator fragments packed side by side;
 *   bo float [cs];   ln_w, ln_b float [cs] zero-padded. */
I2R_API int i2r_hrt_attn_block(const float* x, float* out, const float* ln_w, const float* ln_b, const void* wqkv, const float* bqkv,
                       const void* wo, const float* bo, int32_t n_img, int32_t h, int32_t w, int32_t c, int32_t cs, int32_t heads,
                       float eps, int32_t dtype, int32_t variant, void* stream);

/* i2r_hrt_mlp_block -- 16-bit modes only: the MLP half of a GeneralTransformerBlock in ONE launch,
 *     out = x + GELU(BN3(fc2( GELU(BN2(dw3x3( GELU(BN1(fc1( LayerNorm(x) ))) ))) )))      (hrformer.py:1237, MlpDWBN :1094-1119; same
 * semantics as i2r_layernorm + i2r_conv(fc1, GELU) + i2r_dwconv3x3(GELU) + i2r_conv(fc2, GELU, res_post = x)), one workgroup per 8x6
 * pixel tile (+ halo of 1, recomputed) on v_mfma_f32_16x16x32_{bf16,f16}; the 4C-wide hidden tensor only exists in LDS, 16 channels per
 * wave at a time.  x and out: fp32 NHWC [n, h, w, cs], distinct buffers; pad channels of x must be zero (they are everywhere in this library).
 * (c, cs) = (78, 80), (156, 160) or (312, 320); hidden_pad = 4 cs (zero weights / biases beyond 4c).
 * variant: 0 = the library's choice; 1 = every wave accumulates fc2 over its own hidden blocks for all output blocks, partial sums meet
 * once through LDS (rounds 3-4; 78 / 156); 2 = ten waves per tile, the hidden dimension in rounds of ten block pairs whose packed
 * depth-wise outputs meet in LDS, every wave accumulating ITS output blocks (round 5; 156 / 312).  Same operands and arithmetic.
 * w1: 16-bit 32-deep fragments [hidden_pad/16][cs/32 rounded up][64 lanes][8] of the BN-folded fc1 matrix [hidden, c] (fragment layout as
 * in i2r_hrt_attn_block; columns zero beyond cs), b1 float [hidden_pad]; wdw float [9][hidden_pad] tap-major BN-folded depth-wise
 * weights, bdw [hidden_pad]; w2: fragments [cs/16][hidden_pad/32][64][8] of the BN-folded fc2 matrix [c, hidden] with the hidden columns
 * of every 32-column k-step in slot order (slot 8g + 4h + r <- column 16 (2 kstep + h) + 4g + r), b2 float [cs]. */
I2R_API int i2r_hrt_mlp_block(const float* x, float* out, const float* ln_w, const float* ln_b, const void* w1, const float* b1,
                      const float* wdw, const float* bdw, const void* w2, const float* b2, int32_t n_img, int32_t h, int32_t w,
                      int32_t c, int32_t cs, int32_t hidden_pad, float eps, int32_t dtype, int32_t variant, void* stream);

/* i2r_dwconv3x3 -- depth-wise 3x3 conv, pad 1, stride 1|2, + bias (eval BN folded) + activation (0 none, 1 ReLU,
 * 2 GELU): MlpDWBN.dw3x3+norm2+act2 (hrformer.py:1070-1080,1106-1108) and the DW down-sampling hops of the fuse
 * layers (:1651-1704). w: [9][cs] (tap-major), bias [cs]. */
I2R_API int i2r_dwconv3x3(const float* in, const float* w, const float* bias, float* out, int32_t n_img, int32_t in_h, int32_t in_w,
                  int32_t c, int32_t cs, int32_t stride, int32_t act, int32_t dt /* storage of in and out: 0 fp32, 1 bf16, 2 f16 (stride 1) */,
                  void* stream);

/* i2r_upsample_bilinear_add -- out = act(res + F.interpolate(low, scale_factor=scale, mode='bilinear',
 * align_corners=False)): the up-sampling terms of HighResolutionTransformerModule.forward (hrformer.py:1629-1646,
 * 1718-1730). res may alias out. */
I2R_API int i2r_upsample_bilinear_add(const float* low, const float* res, float* out, int32_t n_img, int32_t low_h, int32_t low_w,
                              int32_t scale, int32_t c, int32_t cs, int32_t act, void* stream);
/* the same with up to three up-sampled terms added in ONE pass, in the order given (a->low2 / a->low3 may be null): the sum of
 * HighResolutionTransformerModule.forward over the lower-resolution branches j > i (hrformer.py:1718-1730) without handing the partial
 * sums through memory; bit-identical to successive i2r_upsample_bilinear_add calls.  All terms share n_img, c, cs; the output is
 * low_h * scale x low_w * scale and every scale divides it.  (i2r_up_args: below, with the program runner's structs.) */
struct i2r_up_args;
I2R_API int i2r_upsample_bilinear_add_multi(const struct i2r_up_args* a, void* stream);

/* i2r_fuse_up_add -- out = act(base + up(t1, s1) [+ up(t2, s2)]), up = nearest-neighbour up-sampling by s (a power of two; t_k is
 * [n, h/s_k, w/s_k, cs]).  The closing step of the HRNet fuse sum for the outputs that receive lower-resolution terms
 * (interformer_pureMulti.py:392-410: y_i = ReLU(x_i + sum_j Upsample(BN(conv1x1(x_j))))): the 1x1 convs write their small maps once
 * and this HBM-bound pass adds them, instead of s x s read-modify-write scatters from the conv epilogues.  The sum is evaluated
 * left to right ((base + t1) + t2).  base may alias out; t2 may be null.  dt: storage type of all tensors (0 fp32, 1 bf16, 2 f16). */
I2R_API int i2r_fuse_up_add(const float* base, const float* t1, int32_t s1, const float* t2, int32_t s2, float* out, int32_t n_img,
                    int32_t h, int32_t w, int32_t cs, int32_t act, int32_t dt, void* stream);

/* i2r_conv1x1_pair -- two chained 1x1 convolutions over NHWC rows in one launch (fp32):
 *     y = act_a(W_a x + b_a [+ res])     written out, [n_pix, y_cs]
 *     z = act_b(W_b y + b_b)             optional (cb_out = 0: only y), [n_pix, z_cs]
 * Replaces conv3 + bn3 + residual + ReLU of one Bottleneck together with conv1 + bn1 + ReLU of the next (reference lib/models/hrnet.py
 * Bottleneck.forward as used by layer1, interformer_pureMulti.py:69-107, :462-476 _make_layer): y stays in registers between the two
 * GEMMs instead of being written and read back.  w_a / w_b are fragment-packed ([cout / 16][cin / 16][64 lanes][4], engine.pack_frag)
 * with eval BatchNorm folded, b_* the folded biases.  res (optional) is laid out like y.  k_a in {64, 128}; ca_out % 32 == 0;
 * cb_out in {0, 64}; channel strides are multiples of 4 floats.  mt: 16-pixel tiles per wave (1, 2, 4; 0 = default). */
typedef struct i2r_conv1x1_pair_args {
    const float* x; const float* w_a; const float* b_a; const float* res; float* y;
    const float* w_b; const float* b_b; float* z;
    int32_t n_pix, k_a, ca_out, cb_out, x_cs, y_cs, z_cs, relu_a, relu_b, mt;
} i2r_conv1x1_pair_args;
I2R_API int i2r_conv1x1_pair(const i2r_conv1x1_pair_args* a, void* stream);

/* i2r_conv1x1_lp -- 1x1 convolution (+ folded BN) over a small number of NHWC pixel rows on the 16-bit matrix pipe, operands straight
 * from global memory, K split over the four waves of a workgroup:
 *     out = act(W x + bias [+ res1] [+ res2]) [+ res_post]          act: 0 none, 1 ReLU, 2 exact-erf GELU
 * Replaces the single 1x1 convs of the unfused HRFormer-B transformer blocks -- q|k|v and out projections (hrformer.py:1164-1180),
 * MlpDWBN fc1 / fc2 (:1094-1119) -- and of the fuse layers (:1629-1704) where the pixel count is a few thousand and i2r_conv is bound
 * by its per-chunk staging latency.  w: fragment-packed 16-bit [cout_pad / 16][ceil(cin_pad / 32)][64 lanes][8] (engine.pack_frag32:
 * lane (li, g) of fragment (f, c) holds W[16 f + li][32 c + 8 g .. + 8), columns beyond cin_pad zero); bias
 * fp32 [cout_pad]; x fp32 (in_16 = 0, packed on load) or stored in the operand type; out, res1, res_post fp32 or 16 bit (out_16).
 * cout_pad / 16 must be a multiple of 3, 4, 5 or 6; cin_pad >= 64.  res1 / res_post may alias out (in-place accumulation of a fuse sum).  mt: 16-pixel tiles per workgroup (1, 2; 0 = chosen from the grid size). */
typedef struct i2r_conv1x1_lp_args {
    const void* x; const void* w; const float* bias; const void* res1; const void* res_post; void* out;
    int32_t n_pix, cin_pad, cout_pad, x_cs, out_cs, act, dtype, in_16, out_16, mt;
    const void* res2;   /* ABI 14: second pre-activation residual, out = act((W x + bias + res1) + res2) [+ res_post]: the last 1x1 conv of an
                           HRFormer down path that closes a fuse sum (running sum + the branch's own map, hrformer.py:1716-1731) */
} i2r_conv1x1_lp_args;
I2R_API int i2r_conv1x1_lp(const i2r_conv1x1_lp_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * i2r_encoder_desc -- one DETR-style post-norm encoder layer over variable-length token groups
 * (persons of one image attend to each other; no padding, no mask tensor).
 * Replaces: TransformerEncoderLayer.forward_post (interformer_pureMulti.py:192-213; attention.py:61-82;
 * transpose_h.py:189-210) incl. nn.MultiheadAttention (1 head), both LayerNorms and the FFN, plus the
 * pad / key_padding_mask / get_valid_output dance (interformer_pureMulti.py:706-750, utils.py:24-37).
 *
 *   q = ((src+pos) Wq^T + bq) * d^-0.5 ; k = (src+pos) Wk^T + bk ; v = src Wv^T + bv
 *   a = softmax_over_group(q k^T) v ;  x = LN1(src + a Wo^T + bo) ;  out = LN2(x + W2 relu(W1 x + b1) + b2)
 *
 * Token matrix layout: [n_tok, cs] fp32 (cs = padded d, multiple of 16).  Group g owns the contiguous
 * token rows [grp_off[g], grp_off[g+1]).  `pos` has per-token rows when pos_stride_tok = cs, or is a
 * table indexed by (token % pos_period) when pos_period > 0 (TransPose-H sine table).
 * Matrices are the reference's [out][in] nn.Linear weights, zero-padded to cs / dff_pad and FRAGMENT-PACKED: every
 * 16 x 16 block is stored as the MFMA A-operand image in lane order,
 *     packed[((rb*KC + c)*64 + l)*4 + r] = W[16*rb + (l & 15)][16*c + 4*(l >> 4) + r],   KC = cols / 16,
 * so that one 64-lane 16-byte load is 1 KB contiguous (a row-major matrix read in operand order costs 4x the
 * texture-addresser time on gfx950).  i2r_encoder_kv fills K / V^T for the first layer of a stack (fp32 mode: one
 * fragment-packed image per 16-token tile of each group, tiles numbered group by group: <= n_tok/16 + n_grp tiles of
 * 16*cs floats each in kbuf and in vbuf); i2r_encoder_layer consumes them.
 * ------------------------------------------------------------------------------------------------ */
typedef struct i2r_encoder_desc {
    const float* src;      /* [n_tok, cs] */
    const float* pos;      /* optional */
    float* kbuf;           /* workspace, max((n_tok/16 + n_grp) * 16 * cs, cs * n_tok_pad) floats (fp32 / 16-bit mode images) */
    float* vbuf;           /* workspace, same size; n_tok_pad = roundup(n_tok, 64) + 64 */
    float* out;            /* [n_tok, cs] (may not alias src) */
    const int32_t* grp_off;/* device int32 [n_grp + 1] */
    const float* w_in;     /* [3*cs, cs]  (q rows, k rows, v rows; padded), fragment-packed like all four matrices */
    const float* b_in;     /* [3*cs] */
    const float* w_out;    /* [cs, cs] */
    const float* b_out;    /* [cs] */
    const float* ln1_w; const float* ln1_b;  /* [cs] */
    const float* w1;       /* [dff_pad, cs] */
    const float* b1;       /* [dff_pad] */
    const float* w2;       /* [cs, dff_pad] */
    const float* b2;       /* [cs] */
    const float* ln2_w; const float* ln2_b;  /* [cs] */
    int32_t n_tok, n_grp;
    int32_t d;             /* real model dim (LayerNorm width, softmax scale d^-0.5) */
    int32_t cs;            /* padded dim: 96 or 80 */
    int32_t dff_pad;       /* padded feed-forward dim: 192 */
    int32_t pos_period;    /* 0: pos row = token; >0: pos row = token % pos_period */
    int32_t n_qtiles32;    /* sum over groups of ceil(group_len / 32) (host knows the lengths): work items of the two-tile kernel */
    float ln_eps;
    /* 16-bit MFMA mode (dtype 1 bf16 / 2 f16; cs 96 or 80, any group offsets): q-proj, QK^T, PV, out-proj and FFN run on
     * v_mfma_f32_16x16x32 with fp32 accumulation; kbuf / vbuf then hold 16-bit data, one image per 32-token block of a group,
     * blocks numbered group by group (n_qtiles32 of them; the same byte budget is enough).  The model dim is padded to
     * csp = 96 = three 32-feature MFMA steps for BOTH widths (d = 78: zero weights beyond feature 77, rows stay 80 floats in HBM).
     * w_*_lp: the matrices above zero-padded to csp / dff_pad, as 16-bit [out][in] with the columns of every 32-block permuted to
     * new position 8g + 4*half + r  <-  column 32c + 16*half + 4g + r  (g < 4, half < 2, r < 4), fragment-packed. */
    int32_t dtype;
    int32_t n_qtiles16, n_qtiles64;   /* like n_qtiles32 for 16- and 64-query tiles (n_qtiles16 = number of K / V fragments) */
    const void* w_in_lp; const void* w_out_lp; const void* w1_lp; const void* w2_lp;
    /* fp32 mode: fuse the K / V projection of the NEXT layer into this launch (the layer output is still in registers):
     * next_w_in / next_b_in = the next layer's padded in_proj (its k and v rows are used), written to next_kbuf / next_vbuf
     * (layouts as kbuf / vbuf, distinct buffers).  All null = no fusion (then the next layer needs i2r_encoder_kv). */
    const float* next_w_in; const float* next_b_in; float* next_kbuf; float* next_vbuf;
    /* 16-bit mode: the per-feature fp32 vectors padded to csp = 96 and concatenated:
     * b_in[3*csp] | b_out[csp] | ln1_w | ln1_b | b1[dff_pad] | b2[csp] | ln2_w | ln2_b   (9*csp + dff_pad floats) */
    const float* vec_lp;
    /* fp32 mode, optional: scratch of the "partial key split".  A launch with between one and two 16-query tiles per CU (256 < n_qtiles16
     * < 512) handles just enough tiles with TWO workgroups (each over half of the group's keys) that every CU carries two workgroups
     * (csrc/i2r_encoder.hip).  split_ws: 256 * 2 * 1792 floats; split_cnt: 256 int32 hand-off counters: i2r_encoder_kv (the first launch
     * of every stack) zeroes them and every layer launch leaves them zero, so a forward that follows a faulted one starts clean.  The
     * hand-off itself is write-through (sc1 payload stores, drained, then an agent-scope atomic; sc1 loads on the other side).
     * SINGLE-STREAM CONTRACT: launches that share a scratch pair -- i.e. all launches of one i2r_run_program list / one Program --
     * must be stream-ordered; replaying the same list concurrently on two streams pairs partials of different forwards.
     * Both null = one workgroup per tile. */
    float* split_ws; int32_t* split_cnt;
    /* 16-bit mode, long groups (n_qtiles64 >= 512): sum over groups of ceil(group_len / 192) = workgroups of the kernel whose four waves
     * share the K / V stream through LDS (192 queries each); 0 = use the one-wave-per-64-queries kernel */
    int32_t n_qtiles192;
} i2r_encoder_desc;

I2R_API int i2r_encoder_kv(const i2r_encoder_desc* d, void* stream);
I2R_API int i2r_encoder_layer(const i2r_encoder_desc* d, void* stream);
/* i2r_encoder_layer_form -- what i2r_encoder_layer would launch for this descriptor (additive: I2R_ABI_VERSION unchanged); the launcher
 * and this query share one selection.  The descriptor is validated exactly as for a launch.
 * fp32 (dtype 0): *qt = 16-query tiles per workgroup, 2 once n_qtiles32 >= 512, else 1; *ks = 2 for the partial key split (qt 1, scratch
 * given, 32 < ceil(n_qtiles16 / 8) < 64), else 1 -> enc_layer4_k<cs / 16, 12, qt, ks>.
 * 16-bit (dtype 1 / 2): *qt = 16-query fragments per work item -- 12 (four waves share 192 queries: n_qtiles64 >= 512 and
 * n_qtiles192 > 0), 4 (64 queries per wave: n_qtiles64 >= 512), else 1 (16 queries per wave); *ks = 1.
 * *grid (may be null): the workgroup count.  qt and ks are required.  No launch happens. */
I2R_API int i2r_encoder_layer_form(const i2r_encoder_desc* d, int32_t* qt, int32_t* ks, int32_t* grid);

/* i2r_mh_attention -- softmax(q k^T) v of nn.MultiheadAttention with ANY head count over the same variable-length token groups
 * (MODEL.N_HEAD > 1: interformer_pureMulti.py:461,473, transpose_h.py:457,467, interformer_2stage.py:221,233, attention.py:1039; the yacs
 * default is 8, lib/config/default.py:63) -- the attention core of the general encoder layer the host composes for configs the fused
 * single-head post-norm kernels above do not cover (N_HEAD > 1, NORMALIZE_BEFORE with MODEL.NAME interformer: forward_pre,
 * attention.py:84-103): q|k and v come from 1x1 i2r_conv launches over the token rows, out-proj / FFN / LayerNorms likewise.
 *   qk  [n_tok, qk_cs] fp32: q of head h at channels [h*hp, h*hp + hp), k of head h at k_off + the same; q ALREADY scaled by
 *       head_dim^-0.5 (folded into the q rows by the host); hp = head_dim rounded up to a multiple of 16 (<= 256), pad dims exactly 0
 *   v   [n_tok, v_cs], out [n_tok, out_cs]: head h at channels [h*hp, h*hp + hp); out's channels behind heads*hp are written as zeros
 *   grp_off device int32 [n_grp + 1]: group g owns token rows [grp_off[g], grp_off[g+1]) (keys of other groups are never seen: the
 *       reference's pad + key_padding_mask, interformer_pureMulti.py:706-750)
 *   n_qtiles16 / 32 / 64 = sum over groups of ceil(len / 16 | 32 | 64) (the host knows the lengths; the kernel picks its query tile by hp)
 * fp32 matrix pipe, one wave per (query tile, head), no workspace. */
typedef struct i2r_mh_attn_args {
    const float* qk; const float* v; float* out; const int32_t* grp_off;
    int32_t n_grp, heads, hp, k_off, qk_cs, v_cs, out_cs, n_qtiles16, n_qtiles32, n_qtiles64;
    const int32_t* key_len;   /* optional device int32 [n_grp]: group g attends to its FIRST key_len[g] rows only; all its rows stay queries
                                 (padded persons under a key_padding_mask, ATTENTION_TYPE window).  Precondition 1 <= key_len[g] <= length of
                                 group g; the kernel clamps to that range (a device array cannot be validated by the host entry point) */
} i2r_mh_attn_args;
I2R_API int i2r_mh_attention(const i2r_mh_attn_args* a, void* stream);
/* i2r_mh_attention_form -- what i2r_mh_attention would launch for these arguments (additive: I2R_ABI_VERSION unchanged); the launcher and
 * this query share one check and one selection.  The arguments are validated exactly as for a launch (no pointer is dereferenced).
 * *hb = hp / 16 and *nq = 16-query tiles per wave -> enc_mh_attn_k<hb, nq>: nq = 4 (64 queries) for hb <= 2 once n_qtiles64 * heads >= 4096
 * waves, else 2 (32 queries) for hb <= 6 once n_qtiles32 * heads >= 4096, else 1.
 * grid (may be null) [2]: grid[0] = n_qtiles16 / 32 / 64 for nq 1 / 2 / 4, grid[1] = ceil(heads / wpb) with wpb = min(heads, 4) waves (one
 * per head) in a workgroup; *block (may be null) = 64 wpb threads.  hb and nq are required.  No launch happens. */
I2R_API int i2r_mh_attention_form(const i2r_mh_attn_args* a, int32_t* hb, int32_t* nq, int32_t* grid, int32_t* block);

/* Attention maps: the need_weights output of nn.MultiheadAttention -- attn_output_weights averaged over the heads, [batch, L, L]
 * (torch/nn/functional.py multi_head_attention_forward; read by the reference's visualize.py:128-268,270-420 through forward hooks on
 * <stack>.layers[i].self_attn, discarded by validate()).  Per group g (= one batch entry of the reference, L_g tokens):
 *   out[out_off[g] + i * L_g + j] = (1 / heads) sum_h softmax_j(q_h[i] . k_h[j])      i, j < L_g, row-major [L_g, L_g]
 *   qk, grp_off, heads, hp, k_off, qk_cs: exactly as i2r_mh_attention reads them (q already scaled by head_dim^-0.5, pad dims 0)
 *   out_off  device int64 [n_grp]: float offset of group g's block (sum L_g^2 exceeds 2^31 floats for large TransPose-H batches)
 *   ws       device workspace of ws_stride floats per token row (rows up to grp_off[n_grp]); ws_stride >= 2 * heads * ceil(max L_g / 128)
 *   n_tiles  = sum over the n_grp groups of ceil(L_g / 16) * ceil(L_g / 128): one wave per (16-query tile, 128-key block)
 * Only the first n_grp groups are computed; nothing outside their blocks is written.  Two launches (row statistics per key block, then
 * the normalised probabilities), fp32 matrix pipe, exp2-based softmax with fp32 statistics, heads summed in a fixed order: deterministic. */
typedef struct i2r_attn_weights_args {
    const float* qk; float* out; const int32_t* grp_off; const int64_t* out_off; float* ws;
    int32_t n_grp, heads, hp, k_off, qk_cs, n_tiles, ws_stride;
} i2r_attn_weights_args;
I2R_API int i2r_attn_weights(const i2r_attn_weights_args* a, void* stream);

/* Attention maps at query points: what visualize.py reads of the maps above -- per query point one row (mode 0, "dependency":
 * attn_map[y, x, :, :], :186-233) or one column (mode 1, "affect": attn_map[:, :, y, x], :333-388) of P = (1 / heads) sum_h softmax_j(q_h[i] .
 * k_h[j]), optionally through F.interpolate(scale_factor=scale, mode="bilinear") -- without ever building [L_g, L_g].  Per group g:
 *   mode 0: raw[k, j] = P[q_tok[g, k], j]        mode 1: raw[k, i] = P[i, q_tok[g, k]]        k < K_g, row-major [K_g, L_g]
 *   scale == 1: out[out_off[g] + k * L_g + j] = raw[k, j]
 *   scale  > 1: L_g = P_g h w; every raw row is P_g maps [h, w]; out block = [K_g, P_g, h scale, w scale], bilinear with
 *               align_corners=False: source coordinate (dst + 0.5) / scale - 0.5 clamped at 0, neighbours clamped at the edge, fp32
 *   qk, grp_off, heads, hp, k_off, qk_cs, out_off: exactly as i2r_attn_weights reads them
 *   q_tok    device int32 [n_grp, K]: token indices inside the group (duplicates allowed).  A negative entry gives an all-zero row.
 *            Precondition q_tok < L_g; the kernel clamps (a device array cannot be validated by the host entry point, cf. key_len)
 *   q_cnt    optional device int32 [n_grp]: group g uses its first K_g = q_cnt[g] entries (clamped to [0, K]); NULL: K_g = K
 *   ws       mode 0: ws_stride floats per (group, entry): n_grp * K rows; mode 1: ws_stride floats per token row, as i2r_attn_weights;
 *            ws_stride >= 2 * heads * ceil(max L_g / 128)
 *   rows     scale > 1 only: device workspace of K * grp_off[n_grp] floats (the raw rows before up-sampling)
 *   grp_off_host  scale > 1 only: HOST copy of grp_off[0 .. n_grp] (every L_g must be a multiple of h w: checked here, and it sizes the
 *            up-sampling grid; the kernels themselves read the device table only)
 *   n_tiles  mode 0: sum over groups of ceil(K_g / 16) * ceil(L_g / 128); mode 1: as i2r_attn_weights
 *   n_col_tiles  mode 1: sum over groups of ceil(L_g / 16) * ceil(K_g / 16)
 * Only the first n_grp groups are computed; nothing outside their blocks is written.  Mode 0: row statistics of the K gathered rows, then
 * a GEMM whose query side is gathered; mode 1: the statistics pass of i2r_attn_weights, then a GEMM whose key side is gathered, each
 * column written as a contiguous vector; then the up-sampling pass.  fp32 matrix pipe, exp2-based softmax with fp32 statistics, heads
 * summed in a fixed order, no atomics: deterministic.  I2R_E_ARG: null pointers, mode outside {0, 1}, scale < 1 or > 64, K < 1 or
 * >= 2^20, n_grp outside 1 .. 65535, the heads / hp / stride / alignment conditions of i2r_attn_weights, and when scale > 1: h or w
 * < 1, h w not dividing a group length (host table).  An empty group is skipped at every scale. */
typedef struct i2r_attn_query_args {
    const float* qk; float* out; const int32_t* grp_off; const int64_t* out_off; float* ws; const int32_t* q_tok; const int32_t* q_cnt;
    float* rows; const int32_t* grp_off_host;
    int32_t n_grp, heads, hp, k_off, qk_cs, n_tiles, ws_stride, mode, K, scale, h, w, n_col_tiles, reserved;
} i2r_attn_query_args;
I2R_API int i2r_attn_query_maps(const i2r_attn_query_args* a, void* stream);

/* Attention per person: the maps above reduced over the persons of an inter-human group, without ever building [L_g, L_g] (additive:
 * I2R_ABI_VERSION unchanged).  Group g = one image: L_g = P_g seg tokens, token (person p, y, x) = p seg + y w + x; P as i2r_attn_weights
 * defines it.  Per group:
 *   dependency  D[i, k] = (1 / seg) sum_{q in person i} P[q, k]     [P_g, L_g]: where person i looks; every row sums to 1
 *   affect      F[j, q] = sum_{k in person j} P[q, k]               [P_g, L_g]: the share of token q's attention on person j; sum_j = 1
 *   relation    R[i, j] = (1 / seg) sum_{q in person i} F[j, q]     [P_g, P_g]: every row sums to 1
 *   rel[rel_off[g] + i P_g + j] = R[i, j], always; mode 1: the maps block of group g holds D, mode 2: F, mode 0: maps is not touched
 *   scale == 1: maps[maps_off[g] + p L_g + t] = D / F[p, t]
 *   scale  > 1: seg = h w; every row is P_g maps [h, w]; maps block = [P_g, P_g, h scale, w scale], the bilinear up-sampling of
 *               i2r_attn_query_maps
 *   qk, grp_off, heads, hp, k_off, qk_cs, ws, ws_stride: exactly as i2r_attn_weights reads them
 *   rel_off, maps_off  device int64 [n_grp]: float offsets of the groups' blocks (maps, maps_off: may be NULL in mode 0)
 *   rows     device workspace of Pmax * grp_off[n_grp] floats, Pmax = max L_g / seg (F, which R is reduced from in every mode; mode 2 at
 *            scale 1 writes F straight into maps and leaves rows alone); twice that for mode 1 at scale > 1 (the raw D rows behind F)
 *   grp_off_host  HOST copy of grp_off[0 .. n_grp], always: every L_g must be a multiple of seg (checked here), and it sizes the launches
 * Only the first n_grp groups are computed; an empty group is skipped; nothing outside the computed groups' blocks is written.  Passes:
 * the statistics pass of i2r_attn_weights; F, one wave per (16-query tile, person j) over j's key tiles (a person boundary may lie
 * inside a key tile or a 128-key block: masked); mode 1: D, one wave per (person i, 32-key block) over i's query tiles; R from F; then
 * the up-sampling pass.  fp32 matrix pipe, fixed summation orders, no atomics: deterministic.  I2R_E_ARG: null pointers, mode outside
 * {0, 1, 2}, scale < 1 or > 64, seg < 1, n_grp outside 1 .. 65535, a group length that seg does not divide, scale > 1 with seg != h w,
 * ws_stride < 2 heads ceil(max L_g / 128), and the heads / hp / stride / alignment conditions of i2r_attn_weights. */
typedef struct i2r_attn_person_args {
    const float* qk; const int32_t* grp_off; float* ws; float* rel; const int64_t* rel_off; float* maps; const int64_t* maps_off;
    float* rows; const int32_t* grp_off_host;
    int32_t n_grp, heads, hp, k_off, qk_cs, ws_stride, seg, mode, scale, h, w, reserved;
} i2r_attn_person_args;
I2R_API int i2r_attn_person_maps(const i2r_attn_person_args* a, void* stream);

/* The target form of the maps per person (additive: I2R_ABI_VERSION unchanged): what grouped inference (PATCH_MODE main_target) needs of
 * them.  Group g holds m_g = L_g / seg members; member 0, tokens [0, seg), is the TARGET, the only member whose output is kept, so only
 * its query rows are computed.  With P, F, D, R as i2r_attn_person_maps defines them:
 *   affect      F_t[j, q] = sum_{k in member j} P[q, k], q < seg        [m_g, seg]: which of the target's tokens look at member j; sum_j = 1
 *   dependency  D_t[k]    = (1 / seg) sum_{q < seg} P[q, k] = D[0, k]   [L_g] = m_g maps [h, w]: where the target looks; sums to 1
 *   relation    r[j]      = (1 / seg) sum_{q < seg} F_t[j, q] = R[0, j] [m_g]: sums to 1
 *   rel[rel_off[g] + j] = r[j], always; mode 1: the maps block of group g holds D_t, mode 2: F_t, mode 0: maps is not touched
 *   scale == 1: maps[maps_off[g] + t] = D_t[t]  /  maps[maps_off[g] + j seg + q] = F_t[j, q]     (L_g floats either way)
 *   scale  > 1: seg = h w; the block is m_g maps [h, w] -> [m_g, h scale, w scale], the bilinear up-sampling of i2r_attn_query_maps
 *   qk, grp_off, heads, hp, k_off, qk_cs, ws, ws_stride, seg, scale, h, w, grp_off_host: exactly as i2r_attn_person_maps reads them
 *            (ws: ws_stride floats per token row, rows up to grp_off[n_grp]; only the targets' rows are written and read)
 *   rel_off, maps_off  device int64 [n_grp]: float offsets of the groups' blocks (m_g floats / L_g scale^2 floats; maps, maps_off: may
 *            be NULL in mode 0)
 *   rows     device workspace of grp_off[n_grp] floats: F_t of group g, [m_g, seg], at rows + grp_off[g] (r is reduced from it in every
 *            mode; mode 2 at scale 1 writes F_t straight into maps and leaves rows alone); twice that for mode 1 at scale > 1 (the raw
 *            D_t of group g at rows + grp_off[n_grp] + grp_off[g])
 * Only the first n_grp groups are computed; an empty group is skipped; nothing outside the computed groups' blocks is written.  Passes,
 * one wave per work item: statistics (target 16-query tile, 128-key block) -- ceil(seg / 16) ceil(L_g / 128) per group; F_t (target
 * 16-query tile, member j) -- ceil(seg / 16) m_g; mode 1: D_t (32-key block) -- ceil(L_g / 32); r (member j) -- m_g; then the
 * up-sampling pass.  These are the person-0 / q < seg work items of i2r_attn_person_maps through the same device functions in the same
 * head, tile and lane orders: at scale 1 rel, D_t and F_t are bit-identical to R[0, :], D[0, :] and F[:, 0:seg] of that call.  fp32
 * matrix pipe, no LDS, no atomics: deterministic.  I2R_E_ARG (nothing is launched): null pointers, mode outside {0, 1, 2}, scale < 1 or
 * > 64, seg < 1, n_grp outside 1 .. 65535, a group length that seg does not divide, scale > 1 with seg != h w, ws_stride < 2 heads
 * ceil(max L_g / 128), and the heads / hp / stride / alignment conditions of i2r_attn_weights. */
typedef struct i2r_attn_target_args {
    const float* qk; const int32_t* grp_off; float* ws; float* rel; const int64_t* rel_off; float* maps; const int64_t* maps_off;
    float* rows; const int32_t* grp_off_host;
    int32_t n_grp, heads, hp, k_off, qk_cs, ws_stride, seg, mode, scale, h, w, reserved;
} i2r_attn_target_args;
I2R_API int i2r_attn_target_maps(const i2r_attn_target_args* a, void* stream);

/* The maps above under the flip test (additive: I2R_ABI_VERSION unchanged).  A stack group has tokens (p, y, x), t = p h w + y w + x; the
 * mirror is mu(p, y, x) = (p, y, w - 1 - x), mu(t) = t - 2 (t mod w) + w - 1.  With P the map of a group in the plain pass and P' the map of
 * the same group in the mirrored pass, the merged map is M[q, k] = (P[q, k] + P'[mu(q), mu(k)]) / 2.  The caller runs i2r_attn_query_maps /
 * i2r_attn_person_maps at scale 1 twice -- on the plain groups, and on the mirrored groups with the table i2r_token_mirror made -- and
 * i2r_attn_flip_merge un-mirrors the remaining (map) axis of the second set, merges and up-samples:
 *   a, b     the raw row blocks of the plain / the mirrored pass: group g's block [rows_g, L_g] row-major at a + src_off[g] and b + src_off[g]
 *            (the scale-1 layout of the two entry points above), L_g = P_g h w
 *   rows_g   seg > 0: L_g / seg (the per-person maps); seg == 0: q_cnt[g] clamped to [0, K], K without q_cnt (the query maps)
 *   out      group g's block [rows_g, P_g, h scale, w scale] at out + out_off[g]: the bilinear up-sampling of i2r_attn_query_maps applied to
 *            m[r, p, y, x] = (a[r, p, y, x] + b[r, p, y, w - 1 - x]) / 2 (one rounded add, an exact halving); scale == 1: m itself
 *   grp_off  device int32 [n_grp + 1]; src_off, out_off device int64 [n_grp]; q_cnt optional device int32 [n_grp]
 *   grp_off_host  HOST copy of grp_off[0 .. n_grp], always: it is checked here and sizes the grid
 * One thread per 4 consecutive outputs, no LDS, no atomics: deterministic.  An empty group is skipped; nothing outside the computed groups'
 * blocks is written.  w == 1 and odd w are served (the centre column maps to itself).  I2R_E_ARG (nothing is launched): null pointers,
 * scale outside 1 .. 64, h or w < 1, seg < 0, seg == 0 with K < 1 or >= 2^20, n_grp outside 1 .. 65535, a group length that h w (or seg)
 * does not divide. */
typedef struct i2r_attn_flip_merge_args {
    const float* a; const float* b; float* out; const int32_t* grp_off; const int64_t* src_off; const int64_t* out_off; const int32_t* q_cnt;
    const int32_t* grp_off_host;
    int32_t n_grp, K, seg, scale, h, w;
} i2r_attn_flip_merge_args;
I2R_API int i2r_attn_flip_merge(const i2r_attn_flip_merge_args* a, void* stream);

/* Attention roll-out (Abnar & Zuidema 2020): a soft-max map APPLIED to a thin matrix, the one step the relations through all encoder
 * layers are chained from, without ever building [L_g, L_g] (additive: I2R_ABI_VERSION unchanged).  Take a stack with captured layers
 * lo .. hi, a contiguous range; P_l is the head-averaged softmax(q k^T) of layer l, exactly what i2r_attn_weights defines:
 *   A_l = (1 - alpha) I + alpha P_l          alpha in [0, 1]
 *   T   = A_hi A_hi-1 ... A_lo               (rows sum to 1)
 * T[q, k] is how much output token q of layer hi draws on input token k of layer lo.  All working matrices are X [K_g, L_g], row-major,
 * fp32, per group: the scale-1 layout of i2r_attn_query_maps.  One STEP (this call, on the q|k of one layer) is
 *   side 0:  X' = (1 - alpha) X + alpha X P_l            side 1:  X' = (1 - alpha) X + alpha X P_l^T
 *   result                                              seed X_0                                      side  layer order
 *   dependency rows at query tokens, T[q, :]            one-hot row at q (negative token: zero row)    0     hi -> lo
 *   affect columns at query tokens, T[:, q]             the same                                       1     lo -> hi
 *   per person dependency D_T[i, k] = mean_{q in i} T[q, k]   row i = 1 / seg on person i's tokens     0     hi -> lo
 *   per person affect F_T[j, q] = sum_{k in j} T[q, k]        row j = 1 on person j's tokens           1     lo -> hi
 *   relation R_T[i, j] = sum_{k in j} D_T[i, k] = mean_{q in i} F_T[j, q] (from whichever chain ran)
 *   qk, grp_off, ws, ws_stride, heads, hp, k_off, qk_cs, n_grp: exactly as i2r_attn_weights reads them (ws: ws_stride floats per token row)
 *   in, out  group g's [K_g, L_g] block at in + x_off[g] and out + x_off[g]; x_off device int64 [n_grp]; in != out
 *   K_g      seg > 0: L_g / seg; seg == 0: q_cnt[g] (optional device int32 [n_grp]) clamped to [0, K], K without q_cnt -- as
 *            i2r_attn_flip_merge counts its rows
 *   scale, h, w, rows: as in i2r_attn_query_maps -- scale > 1 (the LAST step of a chain): the raw rows go to the workspace rows
 *            (K * grp_off[n_grp] floats; seg > 0: max K_g in place of K) and group g's [K_g, P_g, h scale, w scale] block, the bilinear
 *            up-sampling of i2r_attn_query_maps, to out + out_off[g]; out_off device int64 [n_grp], NULL = x_off (scale 1 only)
 *   grp_off_host  HOST copy of grp_off[0 .. n_grp], always: it is checked here and sizes the launches
 * Passes: the statistics pass of i2r_attn_weights; one product pass, one workgroup of 8 waves per (16 output columns, 64 rows of X), which
 * recomputes the map's entries on the fp32 matrix pipe and feeds each probability fragment straight back as an operand against the
 * matching 4-wide slice of X (side 1: the S^T fragments of i2r_attn_weights; side 0: the S fragments of the column form); then the
 * up-sampling pass.  Heads are summed in a fixed order; wave w walks every 8th piece of the reduction dimension in ascending order and
 * the partial sums are added in wave order (a fixed-order combine through LDS), no atomics: deterministic.  An
 * empty group is skipped; nothing outside the computed groups' blocks is written; a zero row of in gives a zero row of out; alpha == 0
 * copies in bit for bit.  I2R_E_ARG (nothing is launched): null pointers, in == out, side outside {0, 1}, alpha outside [0, 1] (NaN too),
 * scale outside 1 .. 64, seg < 0, seg == 0 with K < 1 or >= 2^20, n_grp outside 1 .. 65535, a group length that seg (or, at scale > 1,
 * h w) does not divide, scale > 1 without rows / out_off or with h or w < 1, ws_stride < 2 heads ceil(max L_g / 128), and the heads / hp /
 * stride / alignment conditions of i2r_attn_weights. */
typedef struct i2r_attn_rollout_args {
    const float* qk; const float* in; float* out; const int32_t* grp_off; const int64_t* x_off; const int64_t* out_off; float* ws;
    const int32_t* q_cnt; float* rows; const int32_t* grp_off_host;
    int32_t n_grp, heads, hp, k_off, qk_cs, ws_stride, K, seg, side, scale, h, w;
    float alpha; int32_t reserved;
} i2r_attn_rollout_args;
I2R_API int i2r_attn_rollout_step(const i2r_attn_rollout_args* a, void* stream);

/* i2r_token_mirror -- dst[i] = mu(src[i]) for the n entries of a device int32 token table whose token maps are w wide; a negative entry
 * (a skip) is kept.  src and dst are two tables.  n == 0 returns I2R_OK without a launch.  I2R_E_ARG: a null pointer, n < 0, w < 1. */
I2R_API int i2r_token_mirror(const int32_t* src, int32_t* dst, int64_t n, int32_t w, void* stream);

/* MODEL.ATTENTION_TYPE != 'default' (MODEL.NAME interformer: attention.py:991-1031,1046-1062) -- the inter-human "encoder" is ONE
 * GeneralTransformerBlock: a multi-head attention (q / k / v / out projections with bias, MHA_ :494-835; the relative position bias is
 * gathered but its addition is commented out, :780-786) over the (person, y, x) tokens of an image INCLUDING the padded persons' rows
 * (zero features, keys masked), no residual / FFN / norm, whose [L, B, C] output is then RE-VIEWED: permute(0, 2, 1).contiguous()
 * .view(B, C, P, H, W) (:1025-1029).  The two helpers below restate the padding and that view; the projections are i2r_conv launches, the
 * attention i2r_mh_attention with key_len.
 * i2r_rows_gather: out crop i = src crop map[i] (device int32 [n_out]), zeros where map[i] < 0 (padding_tensor, interformer.py:230-249).
 * i2r_view_scramble: o = attention output rows [n_images][max_persons * hw][cs]; out crop s (NHWC [hw, cs], c real channels) = element
 *   (b', p') = (person_map[s] / max_persons, person_map[s] % max_persons) of the re-viewed tensor:
 *   out[s][yx][c'] = o[b][l][cc] with f = ((b' c + c') max_persons + p') hw + yx, b = f % n_images, cc = (f / n_images) % c, l = f / (c n_images). */
I2R_API int i2r_rows_gather(const float* src, float* out, const int32_t* map, int32_t n_out, int32_t floats_per_crop, void* stream);
I2R_API int i2r_view_scramble(const float* o, float* out, const int32_t* person_map, int32_t n_out, int32_t n_images, int32_t max_persons, int32_t c,
                              int32_t cs, int32_t hw, void* stream);
typedef struct i2r_gather_args { const float* src; float* out; const int32_t* map; int32_t n_out, floats_per_crop; } i2r_gather_args;
typedef struct i2r_scramble_args { const float* o; float* out; const int32_t* person_map; int32_t n_out, n_images, max_persons, c, cs, hw; } i2r_scramble_args;

/* i2r_rows_gather_multi: up to I2R_MAX_GATHER_SEGS row gathers in ONE launch -- the hand-over between the per-person and the per-group
 * part of a grouped forward (Engine.forward_groups(share_first_stage=True): pooled features, position rows and first-member features of
 * both flip halves; then the first row of every group).  Per segment: row i of out (i < n_out) = row map[i] of src when
 * 0 <= map[i] < n_src, else a row of ZEROS (-1 and every out-of-range entry alike): the kernel forms no address from an entry it has
 * not checked, so a wrong table costs zero rows, never a read outside src.  map: device int32 [n_out], read when the launch runs (the
 * caller refills it per call).  Rows are row_bytes bytes of any type, copied as 16-byte chunks: row_bytes a positive multiple of 16,
 * src and out 16-byte aligned, rows dense (row i at i * row_bytes).  A segment with n_out == 0 is skipped (its other fields are not
 * read); when every segment is empty nothing is launched and the call returns 0.
 * CALLER'S CONTRACT: the output ranges [out, out + n_out row_bytes) of the segments do not overlap each other or any segment's
 * [src, src + n_src row_bytes); only src == out is checked.
 * Flat 1-D grid, a row served by ceil(row_bytes / 16 KiB) workgroups of equal share (16 B to > 1 MiB rows), a workgroup never straddles
 * two rows; no LDS, no atomics, vector stores only: deterministic.
 * I2R_E_ARG: null a, n_seg outside 0 .. 8, and for a non-empty segment n_out < 0, a null pointer, src == out, n_src < 0, row_bytes not a
 * positive multiple of 16, a misaligned src / out, more than 2^31 - 1 workgroups in all. */
#define I2R_MAX_GATHER_SEGS 8
typedef struct i2r_gather_seg { const void* src; void* out; const int32_t* map; int32_t n_out, n_src; int64_t row_bytes; } i2r_gather_seg;
typedef struct i2r_gather_multi_args { i2r_gather_seg seg[I2R_MAX_GATHER_SEGS /* 8 */]; int32_t n_seg; } i2r_gather_multi_args;
I2R_API int i2r_rows_gather_multi(const i2r_gather_multi_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Program runner: replay a pre-built list of launches from one C call (no per-op host overhead, and
 * capturable into a hipGraph by the caller).  Streams: ops carry a lane id 0..3; lane 0 is `stream`,
 * other lanes are forked/joined with events by I2R_OP_FORK / I2R_OP_JOIN (op.lane = mask of the lanes 1..3 involved).
 * I2R_OP_RECORD / I2R_OP_WAIT (round 6; op.lane = lane | slot << 8, slot 0..7): RECORD puts event 8 + slot on the lane's stream behind
 * everything issued on it so far; WAIT makes the lane's stream wait for the LAST record of that slot (nothing if it was recorded on the
 * same stream).  Point-to-point, so a lane waits only for what its next launch reads, in the order the producers finish: on MI355X
 * a cross-stream wait costs the waiter ~10 us after the producer ends and the all-to-all form ~20 us for three lanes
 * (tools/probe/xstream_latency*.hip) -- the HRFormer fuse layers start the terms of the early lanes under the last lane's blocks.
 * A program with these ops needs an `events` array of 16 entries; RECORD's op.lane also carries the consumer lanes (mask << 16).
 * DEVICE-SIDE FORM: behind an I2R_OP_LANE_FLAGS op (op.args = device int32[64], zeroed once by the caller; NULL = stay with events)
 * FORK / JOIN / RECORD / WAIT become one-wave kernels -- the producer's stream sets flags behind its work, the consumer's stream spins
 * on its flag, clears it and ends (~6 us instead of ~20 us per cross-lane hop).  The caller hands the buffer over ONLY when every lane
 * stream is its own hardware queue (a spinning kernel in front of the kernel that signals it would never end; engine.lane_streams
 * probes this) and never replays two programs that share a buffer at the same time; a wait gives up after 50 ms and sets entry 63 of
 * the buffer instead of hanging the GPU.
 * Op kinds 14 and 18 are reserved (retired: a persistent conv-chain launch and an all-to-all lane barrier); a program holding them is
 * rejected.
 * ------------------------------------------------------------------------------------------------ */
enum {
    I2R_OP_CONV = 1, I2R_OP_STEM = 2, I2R_OP_MAXPOOL = 3, I2R_OP_HEAD = 4,
    I2R_OP_ENC_KV = 5, I2R_OP_ENC_LAYER = 6, I2R_OP_FORK = 7, I2R_OP_JOIN = 8, I2R_OP_CONV_GROUP = 9,
    I2R_OP_LAYERNORM = 10, I2R_OP_WINATTN = 11, I2R_OP_DWCONV = 12, I2R_OP_UPSAMPLE = 13, /* 14: reserved */
    I2R_OP_PE_RES_STEM = 15, I2R_OP_HRT_ATTN = 16, I2R_OP_HRT_MLP = 17, /* 18: reserved */ I2R_OP_FUSE_UP = 19,
    I2R_OP_CONV1X1_PAIR = 20, I2R_OP_CONV1X1_LP = 21, I2R_OP_MH_ATTN = 22, I2R_OP_PE_CAT_VEC = 23, I2R_OP_ROWS_GATHER = 24, I2R_OP_VIEW_SCRAMBLE = 25,
    I2R_OP_RECORD = 26, I2R_OP_WAIT = 27, I2R_OP_LANE_FLAGS = 28, I2R_OP_ATTN_WEIGHTS = 29,
    I2R_OP_ATTN_QUERY = 30,
    I2R_OP_ROWS_GATHER_MULTI = 31, /* args: i2r_gather_multi_args (additive: I2R_ABI_VERSION unchanged) */
    I2R_OP_ATTN_PERSON = 32, /* args: i2r_attn_person_args (additive as well) */
    I2R_OP_ATTN_TARGET = 33 /* args: i2r_attn_target_args (additive as well) */
};

typedef struct i2r_stem_args {
    const float* in; const float* w; const float* bias; float* out;
    int32_t n_img, cin, in_h, in_w, cout, out_cs, n_src, n_valid, out_dt;
} i2r_stem_args;

typedef struct i2r_pe_res_args {
    const float* in; const float* w_pre; const float* w7; const float* bias; float* out;
    int32_t n_img, in_h, in_w, cout, out_cs, n_src, n_valid;
} i2r_pe_res_args;

typedef struct i2r_pool_args {
    const float* in; float* out;
    int32_t n_img, in_h, in_w, c, in_cs, out_cs;
} i2r_pool_args;

typedef struct i2r_head_args {
    const float* in; const float* w; const float* bias; float* out;
    int32_t n_img, h, w_, cin, in_cs, cout;
} i2r_head_args;

typedef struct i2r_ln_args {
    const float* in; const float* w; const float* b; float* out;
    int32_t npix, c, cs; float eps; int32_t out_dt;
} i2r_ln_args;

typedef struct i2r_winattn_args {
    const float* qkv; const float* bias; float* out;
    int32_t n_img, h, w_, c, cs, heads;
} i2r_winattn_args;

typedef struct i2r_hrt_attn_args {
    const float* x; float* out; const float* ln_w; const float* ln_b; const void* wqkv; const float* bqkv; const void* wo; const float* bo;
    int32_t n_img, h, w_, c, cs, heads; float eps; int32_t dtype, variant;
} i2r_hrt_attn_args;

typedef struct i2r_hrt_mlp_args {
    const float* x; float* out; const float* ln_w; const float* ln_b; const void* w1; const float* b1; const float* wdw; const float* bdw;
    const void* w2; const float* b2;
    int32_t n_img, h, w_, c, cs, hidden_pad; float eps; int32_t dtype, variant;
} i2r_hrt_mlp_args;

typedef struct i2r_dw_args {
    const float* in; const float* w; const float* bias; float* out;
    int32_t n_img, in_h, in_w, c, cs, stride, act, dt;
} i2r_dw_args;

typedef struct i2r_up_args {
    const float* low; const float* res; float* out;
    int32_t n_img, low_h, low_w, scale, c, cs, act;
    /* optional further terms (i2r_upsample_bilinear_add_multi): out = act(((res + up(low, scale)) + up(low2, scale2)) + up(low3, scale3)) */
    const float* low2; const float* low3;
    int32_t scale2, scale3;
} i2r_up_args;

typedef struct i2r_fuse_up_args {
    const float* base; const float* t1; const float* t2; float* out;
    int32_t n_img, h, w, cs, s1, s2, act, dt;
} i2r_fuse_up_args;

typedef struct i2r_conv_group_args {
    const i2r_conv_desc* d[I2R_MAX_GROUP];
    const int32_t* block_map;
    int32_t n;
    int32_t map_len;
} i2r_conv_group_args;

typedef struct i2r_op {
    int32_t kind;
    int32_t lane;          /* stream lane 0..3 (FORK/JOIN: bitmask of lanes to fork to / join from) */
    const void* args;      /* host pointer to the matching *_desc / *_args struct */
} i2r_op;

/* streams: array of 4 hipStream_t (lane 0 = the caller's stream); events: array of >= 8 hipEvent_t (16 when the program holds
 * RECORD / WAIT ops) created by the caller with hipEventDisableTiming.  Both may be NULL when every op uses lane 0. */
I2R_API int i2r_run_program(const i2r_op* ops, int32_t n_ops, void* const* streams, void* const* events);
/* The same replay with every LAUNCH timed through caller-owned events (hipEventCreate with timing enabled; entries of sync ops -- FORK /
 * JOIN / RECORD / WAIT / LANE_FLAGS -- are ignored): the launch of op i goes out through hipExtLaunchKernelGGL with t1[i] BOUND to the dispatch (its completion
 * signal carries the kernel's end time; no extra packet, the replay is not slowed down) and, where t0[i] is non-NULL, t0[i] as a marker in
 * front of it (~5 us of stream time).  hipEventElapsedTime(t0[i], t1[i]) is the kernel's own duration IN SITU -- with the program's other
 * lanes and any sibling program in flight; for a launch without a start marker the start is the completion of whatever it waited for (its
 * predecessor on the stream, or the lanes a sync op named), i.e. the t1 of those ops.  tools/probe/event_timing.hip on MI355X, kernels of
 * 20 / 50 us: start + stop 20.9 / 50.9 us at 26.3 / 56.5 us per launch of stream time; stop only 21.4 / 51.4 us between consecutive stops
 * at 21.5 / 51.5 us per launch (= the untimed rate); plain hipEventRecord pairs 23.7 / 53.6 us at 29.0 / 58.8.  A rocprofv3 kernel trace
 * of the same forward is NOT comparable where streams overlap: its host-side interception serialises the part-batch programs
 * (DESIGN.md section 5).  This is the measurement hook of bench.py (per-kernel durations from HIP events on the stream the
 * kernel is launched on); the reference has no counterpart (tools/compute_flops.py:21-32 times whole forwards).
 * t0, t1: n_ops entries each; t1[i] NULL = op i is not timed. */
I2R_API int i2r_run_program_timed(const i2r_op* ops, int32_t n_ops, void* const* streams, void* const* events, void* const* t0,
                                  void* const* t1);

I2R_API int i2r_abi_version(void);
I2R_API const char* i2r_last_error(void);
/* device sanity: returns 0 when device `dev` is gfx950, fills cu_count / lds_bytes if non-NULL */
I2R_API int i2r_device_check(int32_t dev, int32_t* cu_count, int32_t* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* I2R_HIP_H */
