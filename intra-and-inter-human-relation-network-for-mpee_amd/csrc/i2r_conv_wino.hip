// 3x3 stride-1 convolution as Winograd F(2x2, 3x3) on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), gfx950.
//
// Why: the fp32 MFMA runs at the fp32 VECTOR rate (157 TFLOP/s, 1/16 of the 16-bit pipe) and the direct implicit-GEMM kernel
// (i2r_conv.hip) is bound by exactly that pipe; its HBM side sits at 9 % of the roof.  F(2x2, 3x3) computes a 2x2 output tile from
// a 4x4 input tile with 16 multiplies per (cin, cout) pair instead of 36:  Y = A^T [ (G g G^T) . (B^T d B) ] A  -- 2.25x fewer
// MFMAs for the same result (exact in exact arithmetic; in fp32 the rounding differs from the direct sum by a few ulp of the
// partial sums, far inside the 1e-3 parity bar -- tests/test_kernels_gpu.py).  The weights U = G g G^T are transformed once at
// pack time in float64 (engine.Packer.conv) and stored "k4" with the 16 Winograd positions in place of the 9 taps.
//
// Decomposition (one 4-wave workgroup):
//  * M = Winograd tiles.  A FRAGMENT is 16 tiles = 64 output pixels laid out FW x (16/FW) tiles (FW = 8, 4 or 2, chosen per map so
//    that fragments cover the map without waste: 64x48 -> 16x4 px, 32x24 -> 8x8 px, 16x12 -> 4x16 px); a work ITEM is MT
//    consecutive fragments of the flattened (crop, fy, fx) list x NT x 16 output channels.  Every fragment stages its own
//    (2 FH + 2) x (2 FW + 2) input patch, so the fragments of an item may belong to different crops.
//  * wave i (0..3) owns ROW i of the 4x4 Winograd positions: positions (i, 0..3) x MT fragments x NT channel fragments =
//    4 MT NT accumulator tiles.  Row i of  B^T d B  needs only two rows of d: the wave reads 2 x 4 patch pixels per tile from the RAW
//    patch in LDS and does the input transform in registers (8 ds_read_b128 + 32 VALU per fragment and 16-channel step, next to
//    48 MT MFMAs) -- the transformed tensor (3.2x the patch) never exists in LDS.
//  * LDS holds the raw patch of a 16-channel chunk, double-buffered, the next chunk fetched into registers under the current
//    chunk's MFMAs (as in i2r_conv.hip).  Columns are de-interleaved by parity (slot = row * pitch + (x & 1) * half + (x >> 1)) and
//    the pitch is chosen per FW so that the stride-2 tile gathers of a 16-lane ds_read_b128 group hit 16 distinct 16-byte slots.
//  * B operands (U, k-permuted k4 packing) stream from L2 straight into registers one position ahead, as in the direct kernel; in the
//    plain form the order of those loads and of the next chunk's patch loads is pinned (WINO_PASS; tools/wino_sched.py reads the
//    resulting load-to-wait distances off the assembly, tests/test_wino_sched.py holds them).
//  * epilogue: the column half of the output transform (over j) is in-lane; the row half (over i) crosses the four waves: each
//    wave writes its two partial tiles T_i[b] to LDS as [i][b][tile][cout] and every thread then owns (pixel, 4 channels) pieces:
//    three 16-byte LDS reads, bias / residuals / ReLU, one 16-byte store (a quad of lanes = 64 contiguous bytes of one pixel).
//  * Dispatch: one workgroup per RUN of w_seq items of one channel block (w_seq = 1: per item), numbered member by member in XCD bands
//    or in the order of a host-made table.  A run does the member selection, the item decode, the input-side descriptors, the LDS
//    slots and the weight walk once and then works its fragments off one after the other in the same registers (see the run loop).
//  * The kernel is bound by INSTRUCTION ISSUE as much as by the matrix pipe: an item is small (64 pixels x 48 channels x cin =
//    48 MFMAs per wave and 16-channel chunk), and with every memory access and every MFMA compiled out the launch still took 35 of
//    its 78 us (tools/one_conv.py with the -DI2R_TUNING ablation switches: a SIMD issues about one instruction per 4.7 cycles, and
//    the 1450 non-MFMA instructions a wave executed cost as much issue time as its 247 MFMAs cost pipe time).  Hence: item decode
//    through host-made reciprocals on the scalar ALU (no integer divisions), the first MFMA of every accumulator takes a literal
//    zero (no clearing), one fragment in registers at a time at <= 128 of them (4 waves per SIMD; two fragments held at once at 2
//    waves per SIMD measured 89 vs 78 us, a software-pipelined input transform and persistent workgroups walking an item table
//    measured +-0), and short items strung into runs (pairs of 48-channel fragments: -1 % on the whole model; longer runs balance
//    worse over the CUs than they save -- DESIGN.md section 4).
#include "i2r_conv.h"

namespace {

constexpr int kWinoPatchMax = 108;  // patch pixels of a fragment: 6 x 18 (FW = 8 or 2), 10 x 10 (FW = 4)

// FIN: the "fused input" form.  A member with f_t1 set takes  ReLU((in + up(t1)) + up(t2))  as its input -- the closing pass of an
// HRNet fuse layer (fuse_up_add_k, same summation order) folded into the staging -- and writes that map to f_y on the way (the
// block's second conv reads it as its residual): the non-halo pixels of the fragment patches are disjoint and cover the map, and
// all cin channels pass through the staging, so the items of channel block 0 store every value exactly once.  f_y must not alias
// `in`: the halo reads of neighbouring items are not ordered against those stores.  A member without f_t1 runs as in the plain form.
// the members of the launch where the hardware put them: the kernel-argument block, read with scalar loads
typedef const ConvK __attribute__((address_space(4)))* ConvKArg;

// `args`: grp as it lies in the kernel-argument block.  Only a __global__ function knows where its parameters lie, so the two kernels
// below pass it in (wino_args); the body reads the per-fragment descriptor fields through it (see the run loop).
// EPI: the epilogue's form, chosen by the host per launch (i2r_conv_plan.h, wino_form): 1 = bias + ReLU, 2 = bias + res1 + ReLU, with every
// member's channel blocks exact in cout and out_cs -- the two shapes of the HRNet tower -- compiled without a flag test; 0 = the general
// epilogue (any mix of res1 / res2 / res_post / ReLU, tail blocks, the -DI2R_TUNING switches).  The results do not depend on the form, bit for bit.
template <int MT, int NT, bool FIN, int EPI>
__device__ __forceinline__ void conv_wino_body(const ConvGroupK& grp, ConvKArg args) {
    extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wi = __builtin_amdgcn_readfirstlane(tid >> 6);  // Winograd row of this wave
    const int li = lane & 15, g = lane >> 4;

    // ---- the item of this workgroup: entry blockIdx.x of the dispatch table (member << 24 | item index within the member), or
    //      numbered member by member ----
    int bid = blockIdx.x, gi = 0;
    if (grp.blk_map) {
        const int v = __builtin_amdgcn_readfirstlane(grp.blk_map[bid]);
        gi = v >> 24;
        bid = v & 0xFFFFFF;
    } else {
        int start = 0;
#pragma unroll
        for (int i = 0; i < kMaxGroups - 1; ++i)
            if (i + 1 < grp.n && bid >= grp.blk_end[i]) { gi = i + 1; start = grp.blk_end[i]; }
        bid -= start;
    }
    const ConvK& p = grp.g[gi];
    // tuning aid (I2R_CONV_DBG & 8, -DI2R_TUNING builds only): phase time stamps of the workgroup into the buffer passed as res2 (start, and of
    // the run's LAST fragment: passes begin, passes end, stores done)
    const bool stamp = (I2R_DBG(p) & 8) != 0;
    unsigned long long ts0 = 0, ts1 = 0, ts2 = 0;
    if (stamp) ts0 = __builtin_amdgcn_s_memtime();

    // item -> (fragment group wg, output-channel block cb).  Without a table the items of a member are numbered XCD-aware: workgroup b of a
    // launch runs on XCD b % 8 (own L2 each) and the host pads every member to whole rounds of 8, so XCD x = bid % 8 is handed the
    // CONTIGUOUS band of fragment groups x * w_band .. (x + 1) * w_band - 1 (two crops of a 16-crop launch), in order, each with its
    // channel blocks back to back (q = bid / 8: cb = q % n_cblk, group = x * w_band + q / n_cblk): the n_cblk blocks of a fragment and
    // its row / column neighbours read their input patch and halos from ONE L2.  Plain numbering spreads them over the eight XCDs:
    // PMC FETCH_SIZE per launch 27.5 -> 22.4 MB (stage 3, 16 crops), 10.9 -> 7.2 MB (layer1's 64-channel convs); time -0.3 %.
    // (the run's set-up reads the member through its Wino block, prepare_wino's digest of it: neighbouring fields, wide scalar loads)
    const auto& pk = p.wk;
    const int n_cblk = pk.n_cblk;
    const int bq = grp.blk_map ? bid : bid >> 3;
    const int qq = div_r(bq, pk.r_cblk);
    const int cb = bq - qq * n_cblk;
    const int wg = grp.blk_map ? qq : (bid & 7) * pk.w_band + qq;
    // A workgroup is a RUN of w_seq consecutive fragment groups of one channel block, wg * w_seq .. + w_seq - 1, worked off one after the
    // other on ONE set-up: member selection, item decode, the input-side buffer descriptors, LDS slots, gather bases, weight lane offset and
    // walk are computed once (a 3-pass item spends more instructions around its passes than in them).  What names the fragment -- its decode,
    // the global offsets of the staging items, the output pixel -- is redone per fragment from values read afresh (lane_now, ConvKArg): held
    // through the pass loop instead, it does not fit 128 registers.  The run's fragments past w_nfrag do nothing: the trip count is cut
    // here, workgroup-uniform and before the first barrier, like the return for an empty run.
    const int run0 = wg * pk.w_seq;
    const int nrun = min(pk.w_seq, pk.nruns - run0);
    if (nrun <= 0) return;  // (padding of the last band; workgroup-uniform)
    const int fwl = pk.fwlog, FW = 1 << fwl;  // tiles across a fragment
    const int pitch = pk.pitch, half = pk.half, plane = pk.plane;
    const int n_base = cb * NT * 16;

    // ---- staging assignment: item = (fragment, patch pixel, channel group of the 16-channel chunk); the four lanes of a quad
    //      fetch the 64 contiguous bytes of one pixel (quad rule of the texture addresser, see i2r_conv.hip) ----
    constexpr int NIT = (MT * kWinoPatchMax * 4 + 255) / 256;
    // Global accesses go through buffer instructions: a 32-bit per-lane byte offset + a scalar offset that walks the channel chunks,
    // no 64-bit address arithmetic on the vector ALU, and a lane whose offset lies beyond the descriptor's range reads zeros -- which
    // is how the halo outside the image and the unused items are zero-filled without a select per load.
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pk.in), 0, pk.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pk.w), 0, pk.w_bytes, 0x00020000);
    unsigned goff[NIT];  // byte offset of (pixel, channel group) in `in`, kOOB (out of range: reads zeros) outside the image
    int lslot[NIT];      // LDS slot, -1 = no item; fused-input form: + kOwn when the item is an interior (non-halo) pixel of the patch
    constexpr int kOwn = 1 << 30;  // (above every slot; the shift to a byte address drops it)
    // fused input: the same piece of the up-sampled terms sits at (iy >> s, ix >> s) of their (in_h >> s) x (in_w >> s) maps.  A lane
    // outside the image has all three offsets at kOOB and stages ReLU(0 + 0 + 0) = 0: the zero padding needs no select.  The value
    // goes to f_y from the lanes holding an interior (non-halo) pixel (own) in the items of channel block 0: at `goff`, f_y being laid out like `in`
    const bool fin = FIN && p.f_t1 != nullptr, fin2 = fin && p.f_t2 != nullptr;  // (uniform)
    const __amdgpu_buffer_rsrc_t rs_t1 = make_rsrc(fin ? p.f_t1 : nullptr, p.f_bytes1), rs_t2 = make_rsrc(fin2 ? p.f_t2 : nullptr, p.f_bytes2),
                                 rs_y = make_rsrc(fin ? p.f_y : nullptr, pk.in_bytes);
    unsigned goff1[FIN ? NIT : 1], goff2[FIN ? NIT : 1];
    // The LDS slot of staging item k is the same for every fragment of the run and stays in a register.  Its patch pixel (row, col) is
    // worked out again per fragment, from a thread index the compiler cannot hoist: kept, row / col / offset would hold six more
    // registers through the pass loop, which at 4 waves per SIMD (128 registers) means spills.
    const int cg = tid & 3;  // (256 items per step: the channel group does not depend on k)
    auto patch_pixel = [&](const auto& pq, int t, int k, int& f, int& row, int& col) {  // (pq: the member's Wino block)
        const int PC = pq.pw, PP = pq.pp;
        const int pix = (t + k * 256) >> 2;
        int pp = pix;  // (MT <= 2 and PP <= 108: compare / subtract instead of a division; rows through a 16-bit reciprocal)
        f = 0;
#pragma unroll
        for (int m = 1; m <= MT; ++m)
            if (pix >= m * PP) { f = m; pp = pix - m * PP; }
        row = (pp * pq.w_rcp) >> 16;
        col = pp - row * PC;
    };
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        int f, row, col;
        patch_pixel(pk, tid, k, f, row, col);
        asm volatile("" : "+v"(row), "+v"(col));  // (worked out for every lane: as the arm of a select it becomes a masked block with scalar loads and waits of its own)
        lslot[k] = f < MT ? (f * 4 + cg) * plane + row * pitch + (col & 1) * half + (col >> 1) : -1;
        if constexpr (FIN) {  // (as a bit of the slot, not a lane mask per item: those are four more scalar registers through the pass loop)
            if (f < MT && row >= 1 && row < pk.ph - 1 && col >= 1 && col < pk.pw - 1) lslot[k] |= kOwn;
        }
    }
    // ---- per fragment of the run: decode (scalar) and the global offsets of the staging items ----
    // (the lane index, read where it is used: two instructions, no register held through the passes, nothing hoisted out of the run loop)
    auto lane_now = []() {
        int l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    int f_img[MT], f_oy[MT], f_ox[MT];
    bool f_ok[MT];
    auto set_fragment = [&](int fg, int t, const auto& ps) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            int fid = fg * MT + mt;
            f_ok[mt] = MT == 1 || fid < ps.nfrag;  // (one fragment per group: the run's trip count has cut the groups past the last)
            if (!f_ok[mt]) fid = 0;
            f_img[mt] = div_r(fid, ps.r_img);
            const int rem = fid - f_img[mt] * ps.frags_img;
            const int fy = div_r(rem, ps.r_tx);
            f_oy[mt] = fy * ps.oy_step;
            f_ox[mt] = (rem - fy * ps.tiles_x) * (2 * FW);
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            int f, row, col;
            patch_pixel(ps, t, k, f, row, col);
            int img = f_img[0], oy = f_oy[0], ox = f_ox[0];
            bool ok = f_ok[0] && f < MT;
#pragma unroll
            for (int m = 1; m < MT; ++m)
                if (f == m) { img = f_img[m]; oy = f_oy[m]; ox = f_ox[m]; ok = f_ok[m]; }
            const int iy = oy - 1 + row, ix = ox - 1 + col;
            const bool in_img = ok && (unsigned)iy < (unsigned)ps.in_h && (unsigned)ix < (unsigned)ps.in_w;
            goff[k] = in_img ? (unsigned)(((img * ps.in_h + iy) * ps.in_w + ix) * ps.in_cs + (t & 3) * 4) * 4u : kOOB;
            if constexpr (FIN) {
                const int s1 = ps.f_sh1, s2 = ps.f_sh2;
                goff1[k] = in_img ? (unsigned)(((img * (ps.in_h >> s1) + (iy >> s1)) * (ps.in_w >> s1) + (ix >> s1)) * ps.in_cs + (t & 3) * 4) * 4u : kOOB;
                goff2[k] = in_img ? (unsigned)(((img * (ps.in_h >> s2) + (iy >> s2)) * (ps.in_w >> s2) + (ix >> s2)) * ps.in_cs + (t & 3) * 4) * 4u : kOOB;
            }
        }
    };
    f32x4 v[NIT];
    auto stage_load = [&](int c0) {
#pragma unroll
        for (int k = 0; k < NIT; ++k)
            v[k] = (I2R_DBG(p) & 2) ? (f32x4){0.f, 0.f, 0.f, 0.f}
                                    : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_in, goff[k], c0 * 4, 0));
    };
    // fused input: the first term is fetched with the base piece; the second one takes over its registers half a pass later
    // (stage_mid), after the first has been added -- one extra staging register set instead of two
    f32x4 vt[FIN ? NIT : 1];
    auto stage_load_t1 = [&](int c0) {
        if constexpr (FIN) {
            if (fin) {
#pragma unroll
                for (int k = 0; k < NIT; ++k) vt[k] = buf_ld16(rs_t1, goff1[k], c0 * 4);
            }
        }
    };
    auto stage_mid = [&](int c0) {
        if constexpr (FIN) {
            if (fin2) {
#pragma unroll
                for (int k = 0; k < NIT; ++k) {
                    v[k] += vt[k];
                    vt[k] = buf_ld16(rs_t2, goff2[k], c0 * 4);
                }
            }
        }
    };
    auto stage_store = [&](f32x4* buf, int c0) {
        if constexpr (FIN) {
            if (fin) {
#pragma unroll
                for (int k = 0; k < NIT; ++k) {
                    v[k] += vt[k];
                    v[k][0] = fmaxf(v[k][0], 0.f); v[k][1] = fmaxf(v[k][1], 0.f); v[k][2] = fmaxf(v[k][2], 0.f); v[k][3] = fmaxf(v[k][3], 0.f);
                    if (cb == 0) buf_st16(rs_y, (unsigned)lslot[k] >= (unsigned)kOwn ? goff[k] : kOOB, c0 * 4, v[k]);  // (uniform; no item: goff is kOOB)
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k)
            if (lslot[k] >= 0) buf[FIN ? lslot[k] & (kOwn - 1) : lslot[k]] = v[k];
    };

    // ---- A operand: lane (tile li, channel group g) gathers rows ra, rb of its tile's 4x4 patch and forms row i of B^T d B ----
    //      i = 0: d0 - d2,  1: d1 + d2,  2: d2 - d1,  3: d1 - d3
    const int ra = wi == 0 ? 0 : (wi == 2 ? 2 : 1);
    const int rb = wi == 0 ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
    const float sg = wi == 1 ? 1.f : -1.f;
    const int ty = li >> fwl, tx = li & (FW - 1);
    const int abase = g * plane + 2 * ty * pitch + tx;
    int abase_f;  // (the copy a fragment works with, see the run loop)
    const int oa = ra * pitch, ob = rb * pitch;
    auto load_a = [&](const f32x4* buf, f32x4 (&a)[MT][4]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4* q = buf + mt * 4 * plane + abase_f;
            f32x4 R[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int oc = (c & 1) * half + (c >> 1);
                const f32x4 xa = q[oa + oc], xb = q[ob + oc];
                R[c] = xa + sg * xb;
            }
            a[mt][0] = R[0] - R[2];
            a[mt][1] = R[1] + R[2];
            a[mt][2] = R[2] - R[1];
            a[mt][3] = R[1] - R[3];
        }
    };

    // (the same, column by column, for the scheduled pass of the plain form: R[c] = row ra + sg * row rb of patch column c)
    f32x4 R[MT][4];
    auto gather = [&](const f32x4* buf, int c) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4* q = buf + mt * 4 * plane + abase_f;
            const int oc = (c & 1) * half + (c >> 1);
            const f32x4 xa = q[oa + oc], xb = q[ob + oc];
            R[mt][c] = xa + sg * xb;
        }
    };

    // ---- B operand: U[pos = 4 i + j][cin / 4][cout_pad][4], lane (cout li, g) takes channels 4g..4g+3 of the 16-channel step;
    //      the pointer walks j (stride cin4 * cout_pad slots) and wraps to the next chunk after j = 3 ----
    const unsigned wlane = (unsigned)(n_base + li + g * pk.cout_pad) * 16u;   // per-lane byte offset (constant)
    const int wp0 = wi * pk.w_row;                                            // scalar byte offset of (position 4 i + j, chunk): every
    int wp;                                                                     // fragment of the run walks the same weights from wp0
    const int inc_j = pk.w_inc_j;
    const int inc_wrap = pk.w_inc_wrap;  // from (pass, j = 3) to (pass + 1, j = 0)
    auto fetch_b = [&](f32x4 (&b)[NT]) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            b[nt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane + nt * 256u, (I2R_DBG(p) & 4) ? 0 : wp, 0));
    };

    f32x4 acc[4][MT][NT];
    const int npass = pk.npass;
    const int bufsz = pk.bufsz;
    f32x4 a[MT][4], b0[NT], b1[NT];
    // FIRST: the accumulators do not exist yet -- their first MFMA takes a literal zero as C (no clearing instructions)
#define WINO_MMA(J, B, FIRST)                                                                                   \
    if (!(I2R_DBG(p) & 16))                                                                                     \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt)             \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                                                       \
            acc[J][mt][nt] = mfma16(a[mt][J][s], B[nt][s], ((FIRST) && s == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[J][mt][nt]);
    // ---- the pass: 16 input channels, four positions j of this wave's row, 12 NT MFMAs each ----
    // Fused-input form: the compiler's own order (runtime `more`).  With the staging terms of two more maps in registers the explicit
    // schedule below does not fit the 128 registers of 4 waves per SIMD (it spilled 26 of them), so this form keeps the order it had.
#define WINO_PASS_FIN(PASS, FIRST)                                                               \
    {                                                                                            \
        const int pass_ = (PASS);                                                                \
        f32x4* cur = lds + (pass_ & 1) * bufsz;                                                  \
        f32x4* nxt = lds + ((pass_ + 1) & 1) * bufsz;                                            \
        const bool more = pass_ + 1 < npass;                                                     \
        if (more) { stage_load((pass_ + 1) * 16); stage_load_t1((pass_ + 1) * 16); }             \
        load_a(cur, a);                                                                          \
        wp += inc_j; fetch_b(b1);                                                                \
        WINO_MMA(0, b0, FIRST)                                                                   \
        wp += inc_j; fetch_b(b0);                                                                \
        WINO_MMA(1, b1, FIRST)                                                                   \
        if (more) stage_mid((pass_ + 1) * 16);                                                   \
        wp += inc_j; fetch_b(b1);                                                                \
        WINO_MMA(2, b0, FIRST)                                                                   \
        if (more) { wp += inc_wrap; fetch_b(b0); }                                               \
        WINO_MMA(3, b1, FIRST)                                                                   \
        if (more) stage_store(nxt, (pass_ + 1) * 16);                                            \
        if (!(I2R_DBG(p) & 64)) __syncthreads();                                                 \
    }
    // Plain form: the order of the vector-memory instructions is PINNED (WINO_FENCE: nothing is scheduled across), because the waits
    // count loads in issue order (vmcnt): left to itself the compiler sinks a weight load to its first use to save registers, and then
    // every position starts with a wait for L2, and the first such wait also covers the far patch loads issued ahead of it.
    //   before position 0:  weights of position 1 (b1)                      [b0 came with the previous pass / the set-up]
    //   before position 1:  weights of position 2 (b0), then the next chunk's patch pieces
    //   before position 2:  weights of position 3 (b1)
    //   before position 3:  weights of the next pass's position 0 (b0)
    // So every weight fragment has the 12 NT MFMAs of a whole position to arrive, into registers that position does not read, and
    // the first wait that covers the patch loads is position 3's, 24 MFMAs after their issue (issued at the head of the pass they would
    // be live across all four positions: 8 registers too many).  MORE is a compile-time flag -- the last pass is a copy of its own --
    // because a prefetch in a conditional block makes every wait behind the join count as if it had not been issued: vmcnt(0).
    // The gather is written column by column in the group that can hide it: columns 0 and 2 (position 0) at the head, column 1
    // (positions 1, 2) under position 0, column 3 (position 3) under position 1.  Inside a group the scheduler is free, and it moves
    // the column-1 reads to the end of position 0 (as the parent's order had them); pinning them ahead costs the last two registers.
#define WINO_FENCE __builtin_amdgcn_sched_barrier(0);
#define WINO_A(J, EXPR) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) a[mt][J] = EXPR;
#define WINO_PASS(PASS, FIRST, MORE)                                                             \
    {                                                                                            \
        const int pass_ = (PASS);                                                                \
        asm volatile("; pass: first " #FIRST ", more " #MORE);  /* (keeps the copies apart: merged heads cost spills) */ \
        f32x4* cur = lds + (pass_ & 1) * bufsz;                                                  \
        f32x4* nxt = lds + ((pass_ + 1) & 1) * bufsz;                                            \
        gather(cur, 0); gather(cur, 2);                                                          \
        WINO_A(0, R[mt][0] - R[mt][2])                                                           \
        wp += inc_j; fetch_b(b1);                                                                \
        WINO_FENCE                                                                               \
        gather(cur, 1);                                                                          \
        WINO_MMA(0, b0, FIRST)                                                                   \
        WINO_FENCE                                                                               \
        wp += inc_j; fetch_b(b0);                                                                \
        if (MORE) stage_load((pass_ + 1) * 16);                                                  \
        WINO_FENCE                                                                               \
        WINO_A(1, R[mt][1] + R[mt][2])                                                           \
        gather(cur, 3);                                                                          \
        WINO_MMA(1, b1, FIRST)                                                                   \
        WINO_FENCE                                                                               \
        wp += inc_j; fetch_b(b1);                                                                \
        WINO_FENCE                                                                               \
        WINO_A(2, R[mt][2] - R[mt][1])                                                           \
        WINO_MMA(2, b0, FIRST)                                                                   \
        WINO_FENCE                                                                               \
        if (MORE) { wp += inc_wrap; fetch_b(b0); }                                               \
        WINO_FENCE                                                                               \
        WINO_A(3, R[mt][1] - R[mt][3])                                                           \
        WINO_MMA(3, b1, FIRST)                                                                   \
        WINO_FENCE                                                                               \
        if (MORE) stage_store(nxt, (pass_ + 1) * 16);                                            \
        if (!(I2R_DBG(p) & 64)) __syncthreads();                                                 \
    }
    // ---- output side ----
    float* const Tl = reinterpret_cast<float*>(lds);
    constexpr int TW = NT * 16;                    // floats per tile row of the exchange buffer
    constexpr int TPL = MT * 16 * TW;              // floats per (i, b) plane
    const bool tail = n_base + NT * 16 > p.cout || n_base + NT * 16 > p.out_cs;  // (uniform) the block holds padding channels
    // The epilogue reads its descriptor fields (a dozen scalars and four buffer descriptors) again for every fragment, through a
    // pointer the compiler cannot see through, as set_fragment does: held over the pass loop next to the staging's, they do not fit the
    // scalar registers (the fused-input form spilled eight of them, and three vector registers with them).

    for (int fs = 0; fs < nrun; ++fs) {
    {
        const int tid_s = wi * 64 + lane_now();  // (the thread index again, per fragment; see patch_pixel)
        ConvKArg ps_ = args + gi;
        asm volatile("" : "+s"(ps_));
        set_fragment(run0 + fs, tid_s, ps_->wk);
        // the LDS addresses derived from the slots and the gather base (one per buffer and item) start their lives here, per fragment, as
        // they did per item: hoisted out of the run loop they are eight registers held through the epilogue, and the allocator spills
        if constexpr (FIN) {  // (the fused-input form is at its 128 registers: the gather base is worked out again instead of held through the run)
            const int l = tid_s & 63;
            abase_f = (l >> 4) * plane + 2 * ((l & 15) >> fwl) * pitch + (l & (FW - 1));
        } else {
            abase_f = abase;
            asm volatile("" : "+v"(abase_f));
        }
#pragma unroll
        for (int k = 0; k < NIT; ++k) asm volatile("" : "+v"(lslot[k]));
    }
    wp = wp0;
    stage_load(0);
    stage_load_t1(0);
    if constexpr (FIN) {  // first chunk: the accumulators do not exist yet, so both terms are in flight with the base piece (one latency)
        if (fin2) {
            f32x4 vu[NIT];
#pragma unroll
            for (int k = 0; k < NIT; ++k) vu[k] = buf_ld16(rs_t2, goff2[k], 0);
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                v[k] += vt[k];
                vt[k] = vu[k];
            }
        }
    }
    fetch_b(b0);
    // the exchange buffer of the previous fragment's output transform aliases the staging buffers: its last reads come before this store
    // (the loads above are already in flight under that barrier)
    if (fs) __syncthreads();
    stage_store(lds, 0);
    __syncthreads();
    if (stamp) ts1 = __builtin_amdgcn_s_memtime();
    if constexpr (FIN) {
        WINO_PASS_FIN(0, true)
        for (int pass = 1; pass < npass; ++pass) WINO_PASS_FIN(pass, false)
    } else if (npass == 1) {
        WINO_PASS(0, true, false)
    } else {
        WINO_PASS(0, true, true)
        for (int pass = 1; pass < npass - 1; ++pass) WINO_PASS(pass, false, true)
        WINO_PASS(npass - 1, false, false)
    }
    if (stamp) ts2 = __builtin_amdgcn_s_memtime();

    if constexpr (EPI != 0) {
    // ---- output transform and epilogue, compile-time forms: the arithmetic of the general code below, operation for operation
    //      (T over j in registers, Y over i across the waves, ((u0 + sgn (u1 + u2)) + (bias [+ res1])), max with 0), without its flag
    //      tests.  The Wino block of the member hands over destination, residual, bias and extent side by side (wide scalar loads, one
    //      wait), the two descriptors are formed once, and every bias and residual piece of the fragment is in flight before the
    //      first wait: their sum is taken behind the exchange barrier, where the first of them is needed.
    const int tid_f = wi * 64 + lane_now();
    ConvKArg pe_ = args + gi;
    asm volatile("" : "+s"(pe_));
    const auto& we = pe_->wk;
    const int conv_h = we.conv_h, conv_w = we.conv_w, out_cs = we.out_cs;
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(we.out, 0, we.out_bytes, 0x00020000),
                                 rs_bias = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(we.bias), 0, we.bias_bytes, 0x00020000);
    const int q4 = tid_f & 3, px = tid_f >> 2;  // (pixel and piece as in the general code)
    const bool hi = (px & 2) != 0;
    const int n0 = n_base + q4 * 4;
    float neg1_ = -1.f;
    asm volatile("" : "+s"(neg1_));
    const f32x4 neg1 = {neg1_, neg1_, neg1_, neg1_};
    unsigned obase[MT];
    f32x4 bs[NT], rr[EPI == 2 ? MT : 1][NT];  // (r = bias + res1 is summed where it is used: every piece is in flight before the first wait)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int t = px >> 2;
        const int oy = f_oy[mt] + 2 * (t >> fwl) + (hi ? 1 : 0);
        const int ox = f_ox[mt] + 2 * (t & (FW - 1)) + (px & 1);
        const bool ok = (int)f_ok[mt] & (int)(oy < conv_h) & (int)(ox < conv_w);
        obase[mt] = ok ? (unsigned)(((f_img[mt] * conv_h + oy) * conv_w + ox) * out_cs + n0) * 4u : kOOB;  // (out_h x out_w = conv_h x conv_w)
        if constexpr (EPI == 2) {
            const __amdgpu_buffer_rsrc_t rs_r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(we.res1), 0, we.out_bytes, 0x00020000);
#pragma unroll
            for (int k = 0; k < NT; ++k) rr[mt][k] = buf_ld16(rs_r1, obase[mt] + 64u * k, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 t0 = acc[0][mt][nt] + acc[1][mt][nt] + acc[2][mt][nt];
            // (a - b as fma(b, -1, a): the same rounding, and with a multiplier the compiler cannot see it is a packed instruction, two elements
            //  at a time, where the subtraction of a tile comes out as four scalar ones; the asm keeps the tiles whole for the same reason)
            f32x4 t1 = __builtin_elementwise_fma(acc[3][mt][nt], neg1, __builtin_elementwise_fma(acc[2][mt][nt], neg1, acc[1][mt][nt]));
            asm volatile("" : "+v"(t0), "+v"(t1));
            float* q = Tl + (wi * 2) * TPL + (mt * 16 + ((tid_f & 63) >> 4) * 4) * TW + nt * 16 + (tid_f & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                q[r * TW] = t0[r];
                q[TPL + r * TW] = t1[r];
            }
        }
    // (the bias pieces come from L2 and follow the exchange stores, when the accumulators have left their registers; the residual pieces above
    //  may come from further away and were issued first)
#pragma unroll
    for (int k = 0; k < NT; ++k) bs[k] = buf_ld16(rs_bias, (unsigned)n0 * 4u + 64u * k, 0);
    const float* const tq = Tl + ((px & 1) + (hi ? 2 : 0)) * TPL + (px >> 2) * TW + q4 * 4;
    const float sgn = hi ? -1.f : 1.f;
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float* q = tq + mt * 16 * TW + 16 * k;
            const f32x4 u0 = *reinterpret_cast<const f32x4*>(q);
            const f32x4 u1 = *reinterpret_cast<const f32x4*>(q + 2 * TPL);
            const f32x4 u2 = *reinterpret_cast<const f32x4*>(q + 4 * TPL);
            f32x4 r = bs[k];
            if constexpr (EPI == 2) r += rr[mt][k];
            f32x4 y = u0 + sgn * (u1 + u2) + r;
            y[0] = fmaxf(y[0], 0.f); y[1] = fmaxf(y[1], 0.f); y[2] = fmaxf(y[2], 0.f); y[3] = fmaxf(y[3], 0.f);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), rs_out, obase[mt] + 64u * k, 0, 0);
        }
    } else {
    // ---- output transform.  Over j in registers:  T[0] = m0 + m1 + m2,  T[1] = m1 - m2 - m3 ----
    const int tid_f = wi * 64 + lane_now();  // (the epilogue's index math stays behind the passes, as the staging's stays in set_fragment)
    ConvKArg pe_ = args + gi;
    asm volatile("" : "+s"(pe_));
    const auto& pe = *pe_;
    const float* const res2e = stamp ? nullptr : pe.res2;
    const unsigned out_bytes = pe.out_bytes;
    const __amdgpu_buffer_rsrc_t rs_out = make_rsrc(pe.out, out_bytes), rs_r1 = make_rsrc(pe.res1, out_bytes), rs_r2 = make_rsrc(res2e, out_bytes),
                                 rs_rp = make_rsrc(pe.res_post, out_bytes);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const f32x4 t0 = acc[0][mt][nt] + acc[1][mt][nt] + acc[2][mt][nt];
            const f32x4 t1 = acc[1][mt][nt] - acc[2][mt][nt] - acc[3][mt][nt];
            float* q = Tl + (wi * 2) * TPL + (mt * 16 + ((tid_f & 63) >> 4) * 4) * TW + nt * 16 + (tid_f & 15);  // D layout: rows 4g + r, column li
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                q[r * TW] = t0[r];
                q[TPL + r * TW] = t1[r];
            }
        }
    // ---- over i across the waves:  Y[0][b] = T0 + T1 + T2,  Y[1][b] = T1 - T2 - T3.  A thread owns one output pixel per fragment and
    //      every fourth 16-byte channel piece of it (piece q + 4 k, q = tid & 3: the four lanes of a quad write 64 contiguous bytes), so
    //      the pixel's index math is done once for its NT pieces ----
    // (buffer instructions here too: a pixel outside the map, or a piece in the padding of a tail block, gets the out-of-range offset --
    //  its loads return zeros and its stores are dropped, so the epilogue has no divergent branches)
    unsigned obase[MT];  // byte offset of the pixel's channel n0 in out / res*
    const int q4 = tid_f & 3, px = tid_f >> 2;  // pixel px of the fragment: tile px >> 2, output row parity (px >> 1) & 1, column parity px & 1
    const bool hi = (px & 2) != 0;
    const int n0 = n_base + q4 * 4;  // (+ 16 k < cout_pad: a channel block never reaches past the padded width)
    f32x4 r[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int t = px >> 2;
        const int oy = f_oy[mt] + 2 * (t >> fwl) + (hi ? 1 : 0);
        const int ox = f_ox[mt] + 2 * (t & (FW - 1)) + (px & 1);
        const bool ok = f_ok[mt] && oy < pe.conv_h && ox < pe.conv_w;
        obase[mt] = ok ? (unsigned)(((f_img[mt] * pe.out_h + oy) * pe.out_w + ox) * pe.out_cs + n0) * 4u : kOOB;
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            r[mt][k] = *reinterpret_cast<const f32x4*>(pe.bias + n0 + 16 * k);
            if (!(I2R_DBG(p) & 1)) {
                if (pe.res1) r[mt][k] += buf_ld16(rs_r1, obase[mt] + 64u * k, 0);
                if (res2e) r[mt][k] += buf_ld16(rs_r2, obase[mt] + 64u * k, 0);
            }
        }
    }
    // T0[b] (even output rows) or T1[b] (odd rows) is the first of the three terms; the others follow two planes apart
    const float* const tq = Tl + ((px & 1) + (hi ? 2 : 0)) * TPL + (px >> 2) * TW + q4 * 4;
    const float sgn = hi ? -1.f : 1.f;  // Y = u0 + sgn (u1 + u2)
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            const float* q = tq + mt * 16 * TW + 16 * k;
            const f32x4 u0 = *reinterpret_cast<const f32x4*>(q);             // T0 | T1
            const f32x4 u1 = *reinterpret_cast<const f32x4*>(q + 2 * TPL);   // T1 | T2
            const f32x4 u2 = *reinterpret_cast<const f32x4*>(q + 4 * TPL);   // T2 | T3
            f32x4 y = u0 + sgn * (u1 + u2) + r[mt][k];
            if (pe.relu) { y[0] = fmaxf(y[0], 0.f); y[1] = fmaxf(y[1], 0.f); y[2] = fmaxf(y[2], 0.f); y[3] = fmaxf(y[3], 0.f); }
            unsigned off = obase[mt] + 64u * k;
            if (pe.res_post) y += buf_ld16(rs_rp, off, 0);
            if (tail) {  // (uniform) channels >= cout are padding: keep them exactly zero; pieces beyond the row are not written
                const int n = n0 + 16 * k;
                if (!(n + 4 <= pe.cout || n + 4 <= pe.out_cs)) off = kOOB;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e >= pe.cout) y[e] = 0.f;
            }
            if (!(I2R_DBG(p) & 1) || y[0] == 12345.678f) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), rs_out, off, 0, 0);
        }
    }  // (EPI == 0)
    }  // (fragments of the run)
#undef WINO_PASS
#undef WINO_PASS_FIN
#undef WINO_A
#undef WINO_FENCE
#undef WINO_MMA
    if (stamp) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long ts3 = __builtin_amdgcn_s_memtime();
        if (tid == 0) {
            unsigned long long* o = reinterpret_cast<unsigned long long*>(const_cast<float*>(p.res2)) + (size_t)bid * 4;
            o[0] = ts0; o[1] = ts1; o[2] = ts2; o[3] = ts3;
        }
    }
}

// grp is the FIRST and ONLY parameter of both kernels, passed by value: it starts the kernel-argument block, and its members start grp.
// A kernel with another signature must not use wino_args().
__device__ __forceinline__ ConvKArg wino_args() {
    static_assert(offsetof(ConvGroupK, g) == 0, "the members lead the kernel argument");
    return (ConvKArg)__builtin_amdgcn_kernarg_segment_ptr();
}

template <int MT, int NT, int EPI>
__global__ __launch_bounds__(256, (MT == 1 ? (NT == 3 ? 4 : 3) : 2)) void conv_wino_f32(const ConvGroupK grp) {
    conv_wino_body<MT, NT, false, EPI>(grp, wino_args());
}

// the fused-input form (a grouped launch takes it when a member has f_t1)
template <int MT, int NT, int EPI>
__global__ __launch_bounds__(256, (MT == 1 ? (NT == 3 ? 4 : 3) : 2)) void conv_wino_fin_f32(const ConvGroupK grp) {
    conv_wino_body<MT, NT, true, EPI>(grp, wino_args());
}

template <int NT>
conv_fn pick_form(int fin, int epi) {
    switch (epi + 3 * (fin != 0)) {
        case 0: return conv_wino_f32<1, NT, 0>;
        case 1: return conv_wino_f32<1, NT, 1>;
        case 2: return conv_wino_f32<1, NT, 2>;
        case 3: return conv_wino_fin_f32<1, NT, 0>;
        case 4: return conv_wino_fin_f32<1, NT, 1>;
        case 5: return conv_wino_fin_f32<1, NT, 2>;
    }
    return nullptr;
}

}  // namespace

// epi: the epilogue form 0 / 1 / 2 (conv_wino_body); the names a trace shows carry it as a third template argument
void* i2r_pick_conv_wino(int nt, int mt, int fin, int epi) {
    conv_fn fn = nullptr;
    if (epi < 0 || epi > 2) return nullptr;
    if (mt == 1 && nt == 3) fn = pick_form<3>(fin, epi);
    if (mt == 1 && nt == 4) fn = pick_form<4>(fin, epi);
    return reinterpret_cast<void*>(fn);
}

// LDS bytes of a Winograd workgroup: two raw-patch chunk buffers, re-used by the cross-wave exchange of the output transform
size_t i2r_conv_wino_lds(int nt, int mt, int plane) {
    const size_t stage = (size_t)2 * mt * 4 * plane * 16;
    const size_t xchg = (size_t)4 * 2 * mt * 16 * nt * 16 * 4;
    return stage > xchg ? stage : xchg;
}
