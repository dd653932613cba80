// Fused convolution for gfx950: implicit GEMM on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32).
//
// Design (MI355X-first, see DESIGN.md "conv_igemm_f32"):
//  * activations NHWC fp32; one workgroup (4 waves) owns a TH x TW tile of output pixels x a block of
//    output channels; GEMM M = pixels, N = cout, K = taps x cin.
//  * the input PATCH of the tile (halo included) is staged ONCE per channel chunk into LDS in a
//    channel-group-major image  lds[cg][patch_pixel] (float4 = 4 consecutive channels), so all taps of the
//    filter read it at shifted addresses: im2col happens in the LDS address, HBM/L2 sees each input
//    element once per workgroup.  A fragments are ds_read_b128: lane (pixel = l&15, g = l>>4) reads
//    channels 4g..4g+3 of a 16-channel step -> feeds FOUR consecutive MFMAs (k permuted so that MFMA step s
//    contracts channels {4g+s}); with plane strides that are multiples of 256 B the 16-lane groups of
//    ds_read_b128 hit distinct bank slots.
//  * weights are pre-packed "k4":  w[tap][cin/4][cout_pad][4]  so a B fragment (cout = l&15, g) is one 16-byte
//    global load per 4 MFMAs, streamed from L2 straight to registers (no LDS, no barrier in the K loop);
//    the fp32 MFMA is slow enough (32 cycles) that 1 KiB of L2 traffic per 4*MT MFMAs per wave hides.
//  * epilogue fuses folded-BN bias, up to two residual inputs, ReLU and the nearest-neighbour upsample
//    scatter of the HRNet fuse layers (each destination element is owned by exactly one lane, so
//    accumulating into `out` in place through res1 == out is race-free).
#include "i2r_conv.h"

namespace {

template <int MT, int NT, int CAP, int PF>
__device__ __forceinline__ void conv_body(const ConvK& p, int bid, f32x4* lds) {
    const int tid = threadIdx.x;
    // tuning aid (I2R_CONV_DBG & 8): per-workgroup phase time stamps (s_memtime) into the buffer passed as res2
    unsigned long long ts0 = 0, ts1 = 0, ts2 = 0;
    const bool stamp = (I2R_DBG(p) & 8) != 0;
    const int bid_stamp = bid;
    if (stamp) ts0 = __builtin_amdgcn_s_memtime();
    const int lane = tid & 63, wave = tid >> 6;
    const int WN = p.wn;
    const int wm = wave >> p.wn_log, wn = wave & (WN - 1);
    const int li = lane & 15, g = lane >> 4;

    int q = div_m(bid, p.n_cblk, p.m_cblk);  // (host-made reciprocals: no integer division in the prologue)
    const int cb = bid - q * p.n_cblk;
    bid = q;
    q = div_m(bid, p.tiles_x, p.m_tx);
    const int tile_x = bid - q * p.tiles_x;
    bid = q;
    const int img = div_m(bid, p.tiles_y, p.m_ty);
    const int tile_y = bid - img * p.tiles_y;
    const int oy0 = tile_y * p.tile_h, ox0 = tile_x * p.tile_w;
    const int py0 = oy0 * p.stride + p.iy0, px0 = ox0 * p.stride + p.ix0;
    const int phw = p.ph * p.pw;

    // Staging assignment: thread t handles the patch pixels (t >> 2) + 64 j and, of every 4 consecutive channel groups, group
    // (t & 3) -- the four lanes of a quad fetch the 64 contiguous bytes of ONE pixel.  (With one pixel per lane every lane of
    // a load hits a different 64-byte segment and the texture addresser needs 64 instead of 16 cycles per instruction:
    // tools/probe/load_pattern.hip.)
    // patch pixel -> global float offset of channel 0 (clamped to 0 outside the image, with a validity bit);
    // channel independent, so computed once
    // (the synchronous variant PF == 0 serves patches of up to 1280 pixels: it keeps one pixel per lane, 20 offsets per thread
    // would cost a wave of occupancy)
    // (global accesses are buffer instructions: 32-bit lane byte offsets + scalar chunk offsets, no 64-bit address arithmetic on the
    //  vector ALU; a lane at kOOB -- halo outside the image, unused slots -- reads zeros without a select per load)
    constexpr int NPP = PF > 0 ? 4 * PF : kMaxPP;
    const int ul = tid & 3;
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(p.in, p.in_bytes), rs_in2 = make_rsrc(p.in2, p.in_bytes), rs_w = make_rsrc(p.w, p.w_bytes);
    unsigned goff[NPP];  // byte offset of the patch pixel's channel 0, kOOB outside the image
#pragma unroll
    for (int j = 0; j < NPP; ++j) {
        const int pp = PF > 0 ? (tid >> 2) + j * 64 : tid + j * 256;
        goff[j] = kOOB;
        if (pp < phw) {
            const int py = div_m(pp, p.pw, p.m_pw), px = pp - py * p.pw;
            const int iy = py0 + py, ix = px0 + px;
            if (iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w) goff[j] = (unsigned)(((img * p.in_h + iy) * p.in_w + ix) * p.in_cs) * 4u;
        }
    }
    const int npp = (phw + 255) >> 8;  // PF == 0: patch pixels per thread actually in use (wave-uniform)

    // A-fragment patch-pixel base of this lane's pixel in each M fragment
    const int tile_px = p.tile_h * p.tile_w;
    int ppix[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int m = (wm * MT + mt) * 16 + li;
        if (m >= tile_px) m = 0;  // padded rows compute garbage-free duplicates; masked at the store
        const int ty = div_m(m, p.tile_w, p.m_tw), tx = m - ty * p.tile_w;
        ppix[mt] = ty * p.stride * p.pw + tx * p.stride;
    }

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int n_base = (cb * WN + wn) * NT * 16;
    const int cin4 = p.cin >> 2;
    // lane's weight offset: float4 index ((tap*cin4 + cg) * cout_pad + n): the lane part (n, g) is constant, the rest walks on the scalar ALU
    const unsigned wlane = (unsigned)(n_base + li + g * p.cout_pad) * 16u;

    // ---- one channel chunk: K loop over (tap, 16-channel step) reading the staged patch `buf`, software-pipelined
    //      one step ahead with two named register sets (no register copies, so the compiler's vmcnt/lgkmcnt waits land
    //      at the first use); `mid` runs right after the first operand fetch (used to launch the next chunk's loads) ----
    auto run_chunk = [&](const f32x4* buf, int c0, int ckc, auto&& mid) {
        const int ncs = ckc >> 4;
        const int nit = p.ntaps * ncs;
        const int wp0 = (c0 >> 2) * p.cout_pad * 16;  // step (tap 0, cs 0) of this chunk (scalar byte offset)
        int wp = wp0;
        const int inc_cs = 4 * p.cout_pad * 16;
        const int inc_tap = (cin4 - (ncs - 1) * 4) * p.cout_pad * 16;
        int cs_n = 0, tx_n = 0, ty_n = 0;  // position of the next step to fetch
        auto fetch = [&](f32x4(&a)[MT], f32x4(&b)[NT]) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = buf_ld16(rs_w, wlane + nt * 256u, (I2R_DBG(p) & 4) ? wp0 : wp);
            const int abase = (cs_n * 4 + g) * p.plane + ty_n * p.pw + tx_n;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[mt] = buf[abase + ppix[mt]];
            if (++cs_n == ncs) {
                cs_n = 0;
                wp += inc_tap;
                if (++tx_n == p.tap_kw) {
                    tx_n = 0;
                    if (++ty_n == p.tap_kh) { ty_n = 0; wp = wp0; }  // wrap: the look-ahead past the last step stays in bounds
                }
            } else {
                wp += inc_cs;
            }
        };
        auto fma_step = [&](const f32x4(&a)[MT], const f32x4(&b)[NT]) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(a[mt][s], b[nt][s], acc[mt][nt]);
        };
        f32x4 a0[MT], a1[MT], b0[NT], b1[NT];
        fetch(a0, b0);
        mid();
        int it = 0;
        for (; it + 2 <= nit; it += 2) {
            fetch(a1, b1);
            fma_step(a0, b0);
            fetch(a0, b0);  // unconditional (wraps after the last step) so both halves keep counted waits
            fma_step(a1, b1);
        }
        if (it < nit) fma_step(a0, b0);
    };

    if constexpr (PF > 0) {
        // ---- double-buffered staging: chunks of 4*ckg channels (ckg <= CAP); the NEXT chunk's patch is loaded into
        //      registers while the MFMAs of the current chunk run, and written to the other LDS buffer afterwards
        //      (one barrier per chunk) ----
        constexpr int UQ = CAP / 4, PJ = 4 * PF;
        f32x4 v[UQ][PJ];
        const int ckg = p.ck >> 2;
        auto stage_load = [&](int c0) {
#pragma unroll
            for (int uq = 0; uq < UQ; ++uq)
                if (uq * 4 < ckg) {
#pragma unroll
                    for (int j = 0; j < PJ; ++j)
                        // (predicated on the pixel lying inside the image: halo pixels outside cost no memory access -- and the
                        //  exec-masked loads keep this block of loads together: with unconditional loads the same kernel measured 8 % slower)
                        v[uq][j] = (I2R_DBG(p) & 2) ? (f32x4){0.f, 0.f, 0.f, 0.f} : buf_ld16(rs_in, goff[j] + (uq * 4 + ul) * 16u, c0 * 4);
                }
            if (p.in2) {
#pragma unroll
                for (int uq = 0; uq < UQ; ++uq)
                    if (uq * 4 < ckg) {
#pragma unroll
                        for (int j = 0; j < PJ; ++j)
                            v[uq][j] += buf_ld16(rs_in2, goff[j] + (uq * 4 + ul) * 16u, c0 * 4);
                    }
            }
        };
        auto stage_store = [&](f32x4* buf) {
#pragma unroll
            for (int uq = 0; uq < UQ; ++uq)
                if (uq * 4 < ckg) {
#pragma unroll
                    for (int j = 0; j < PJ; ++j) {
                        const int pp = (tid >> 2) + j * 64;
                        if (pp < phw) buf[(uq * 4 + ul) * p.plane + pp] = v[uq][j];
                    }
                }
        };
        const int npass = p.npass;
        stage_load(0);
        stage_store(lds);
        __syncthreads();
        if (stamp) ts1 = __builtin_amdgcn_s_memtime();
        for (int pass = 0; pass < npass; ++pass) {
            f32x4* cur = lds + (pass & 1) * ckg * p.plane;
            f32x4* nxt = lds + ((pass + 1) & 1) * ckg * p.plane;
            const bool more = pass + 1 < npass;
            run_chunk(cur, pass * p.ck, p.ck, [&]() { if (more) stage_load((pass + 1) * p.ck); });
            if (more) stage_store(nxt);
            __syncthreads();
        }
    } else {
        for (int c0 = 0; c0 < p.cin; c0 += p.ck) {
            const int ckc = min(p.ck, p.cin - c0);
            const int ncg = ckc >> 2;
            if (c0 != 0) __syncthreads();
            // ---- stage the patch: lds[cg][pp] = in[pixel(pp)][c0 + 4cg .. +3]; 4 channel groups per trip so the
            //      global loads of a trip are all in flight before the first LDS store waits for them ----
            for (int cg0 = 0; cg0 < ncg; cg0 += 4) {
                f32x4 v[4][kMaxPP];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < kMaxPP; ++j)
                        v[u][j] = (j < npp && !(I2R_DBG(p) & 2)) ? buf_ld16(rs_in, goff[j] + u * 16u, (c0 + cg0 * 4) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
                if (p.in2) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int j = 0; j < kMaxPP; ++j)
                            if (j < npp) v[u][j] += buf_ld16(rs_in2, goff[j] + u * 16u, (c0 + cg0 * 4) * 4);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < kMaxPP; ++j) {
                        const int pp = tid + j * 256;
                        if (j < npp && pp < phw)
                            lds[(cg0 + u) * p.plane + pp] = v[u][j];
                    }
            }
            __syncthreads();
            run_chunk(lds, c0, ckc, []() {});
        }
    }

    if (stamp) {
        ts2 = __builtin_amdgcn_s_memtime();
        ConvK q = p;
        q.res2 = nullptr;
        conv_epilogue<MT, NT, 0>(q, acc, img, oy0, ox0, wm, n_base, li, g, tile_px);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long ts3 = __builtin_amdgcn_s_memtime();
        if (tid == 0) {
            unsigned long long* o = reinterpret_cast<unsigned long long*>(const_cast<float*>(p.res2)) + (size_t)bid_stamp * 4;
            o[0] = ts0; o[1] = ts1; o[2] = ts2; o[3] = ts3;
            if (I2R_DBG(p) & 32) {  // where did the hardware place this workgroup?  HW_ID (CU / SE / SIMD fields) | XCC_ID << 32
                const unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
                const unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));
                o[1] = ((unsigned long long)xcc << 32) | hw;
            }
        }
        return;
    }
    conv_epilogue<MT, NT, 0>(p, acc, img, oy0, ox0, wm, n_base, li, g, tile_px);
}

// ---- The double-buffered variants (PF > 0) with a pinned chunk pipeline (FORM 1 | 2; FORM 0 is conv_body above, unchanged) ----
// Same arithmetic in the same (chunk, tap, channel step) order and the same epilogue operations as conv_body: the results are equal bit
// for bit (tests/test_conv_direct_forms_gpu.py).  What differs is what a wave issues around its MFMAs:
//  * vmcnt counts loads in ISSUE order.  conv_body issues the next chunk's patch loads behind the first K step's weights and ahead of
//    the second step's, so the wait for the second step's weights, one step later, forces the whole patch too: nothing of its latency
//    is hidden, and `more` being a run-time flag makes the waits behind its join conservative.  Here a chunk is compiled with and without a
//    successor, the order of the vector-memory groups is pinned (CONV_FENCE), and the patch loads are issued in the chunk's TAIL: behind
//    the weights of its last step, with the last two K steps (8 MT NT MFMAs) to arrive under and no weight wait behind them.  The tail
//    is peeled off the two-steps-per-trip loop (2 or 3 steps), so no look-ahead fetch past the last step is issued at all.
//  * SINGLE (FORM 1; the host takes it when every member has one chunk): the staging registers live from the loads to the one LDS store
//    and are not carried through the K loop (conv_body holds the CAP x PF x 4 of them for the prefetch it never makes).
//  * the K-loop walk (weight offset, LDS offset of the step) advances by selected increments on the scalar ALU: no branch per step.
//  * the loop's scalars are read once, ahead of it, and pinned in registers (kernel arguments are otherwise re-read where they are used: a
//    scalar load and an lgkmcnt(0) in the middle of the chunk); staging stores are one compare and one store each.
//  * EPI 1 | 2: the compile-time epilogue forms of i2r_conv.h; their bias / residual pieces are fetched in the LAST chunk's tail (where the
//    patch loads of a further chunk would go) for MT <= 2; with more accumulators the registers for that do not exist, and they are
//    fetched behind the K loop.
// A launch with an in2 member runs conv_body: a second register set for the terms does not fit (CAP 12: 48 more registers, a wave of
// occupancy), and summed right behind the loads, as there, the schedule above gains nothing.
#define CONV_FENCE __builtin_amdgcn_sched_barrier(0);
template <int MT, int NT, int CAP, int PF, bool SINGLE, int EPI>
__device__ __forceinline__ void conv_body_forms(const ConvK& p, int bid, f32x4* lds) {
    static_assert(PF > 0, "the pinned pipeline exists for the double-buffered variants");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int WN = p.wn;
    const int wm = wave >> p.wn_log, wn = wave & (WN - 1);
    const int li = lane & 15, g = lane >> 4;

    int q = div_m(bid, p.n_cblk, p.m_cblk);
    const int cb = bid - q * p.n_cblk;
    bid = q;
    q = div_m(bid, p.tiles_x, p.m_tx);
    const int tile_x = bid - q * p.tiles_x;
    bid = q;
    const int img = div_m(bid, p.tiles_y, p.m_ty);
    const int tile_y = bid - img * p.tiles_y;
    const int oy0 = tile_y * p.tile_h, ox0 = tile_x * p.tile_w;
    const int py0 = oy0 * p.stride + p.iy0, px0 = ox0 * p.stride + p.ix0;
    const int phw = p.ph * p.pw;

    // what the chunk loop reads, read here and kept: no kernel-argument load between the first MFMA and the last
    auto pin = [](int x) __attribute__((always_inline)) { x = __builtin_amdgcn_readfirstlane(x); asm volatile("" : "+s"(x)); return x; };
    const int plane = pin(p.plane), pw = pin(p.pw), tap_kw = pin(p.tap_kw), cout_slots = pin(p.cout_pad * 16);
    const int ck = pin(p.ck), npass = pin(p.npass), ntaps = pin(p.ntaps), cin4 = pin(p.cin >> 2);
    const int ckg = ck >> 2, ncs = ck >> 4, nit = ntaps * ncs;

    // staging assignment as in conv_body: patch pixels (t >> 2) + 64 j, channel groups (t & 3) + 4 uq
    constexpr int UQ = CAP / 4, PJ = 4 * PF;
    const int ul = tid & 3, pp0 = tid >> 2;
    const __amdgpu_buffer_rsrc_t rs_in = make_rsrc(p.in, p.in_bytes), rs_w = make_rsrc(p.w, p.w_bytes);
    unsigned goff[PJ];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        const int pp = pp0 + j * 64;
        goff[j] = kOOB;
        if (pp < phw) {
            const int py = div_m(pp, p.pw, p.m_pw), px = pp - py * p.pw;
            const int iy = py0 + py, ix = px0 + px;
            if (iy >= 0 && iy < p.in_h && ix >= 0 && ix < p.in_w) goff[j] = (unsigned)(((img * p.in_h + iy) * p.in_w + ix) * p.in_cs) * 4u + ul * 16u;
        }
    }
    const int slot0 = ul * plane + pp0;  // LDS slot of (pixel pp0, group ul); pixel j and group block uq: + 64 j + 4 uq plane

    // A-fragment slot of this lane's pixel in each M fragment, channel group g of a step included
    const int tile_px = p.tile_h * p.tile_w;
    int apix[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        int m = (wm * MT + mt) * 16 + li;
        if (m >= tile_px) m = 0;
        const int ty = div_m(m, p.tile_w, p.m_tw), tx = m - ty * p.tile_w;
        apix[mt] = g * plane + ty * p.stride * pw + tx * p.stride;
    }

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int n_base = (cb * WN + wn) * NT * 16;
    const unsigned wlane = (unsigned)(n_base + li + g * p.cout_pad) * 16u;

    // the walk of a chunk's steps (tap row, tap column, channel step): byte offset into the weights, slot offset into the patch
    // (a channel step's increment, plus what a tap step and a row step add to it: sums of selected terms, no select between variables)
    const int w_cs = 4 * cout_slots, w_dtap = (cin4 - ncs * 4) * cout_slots;
    const int a_cs = 4 * plane, a_dtap = 1 - ncs * 4 * plane, a_drow = pw - tap_kw;

    // every load of a chunk is issued whatever ckg is (straight-line code: a load in a conditional block makes the waits behind the join
    // count as if it had not been issued); the groups a member's chunk does not have are sent out of range and read zeros
    unsigned oob[UQ];
#pragma unroll
    for (int uq = 0; uq < UQ; ++uq) oob[uq] = uq * 4 < ckg ? 0u : kOOB;
    f32x4 v[UQ][PJ];
    auto stage_load = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int uq = 0; uq < UQ; ++uq)
#pragma unroll
            for (int j = 0; j < PJ; ++j) v[uq][j] = buf_ld16(rs_in, uq == 0 ? goff[j] : ((goff[j] + uq * 64u) | oob[uq]), c0 * 4);
    };
    auto stage_store = [&](f32x4* buf) __attribute__((always_inline)) {
        // (the pieces are "used" here, all at once: a load whose only use is one masked store is otherwise sunk into that store's block,
        //  where it is issued late and waited for with vmcnt(0))
#pragma unroll
        for (int uq = 0; uq < UQ; ++uq)
#pragma unroll
            for (int j = 0; j < PJ; ++j) asm volatile("" : "+v"(v[uq][j]));
#pragma unroll
        for (int uq = 0; uq < UQ; ++uq)
            if (uq * 4 < ckg) {
                f32x4* q4 = buf + uq * 4 * plane + slot0;
#pragma unroll
                for (int j = 0; j < PJ; ++j)
                    if (pp0 + j * 64 < phw) q4[j * 64] = v[uq][j];
            }
    };

    // ---- the K loop's operands: two named register sets, fetched one step ahead.  The weights (B: L2 -> registers) and the patch (A: LDS ->
    //      registers) walk the steps on counters of their own, because the weights of a chunk's FIRST step do not wait for its patch: they are
    //      issued ahead of the staging store and the barrier (first_b) and arrive under them ----
    f32x4 a0[MT], a1[MT], b0[NT], b1[NT];
    int wp = 0, cs_b = 0;           // weights: byte offset of the next step, its channel step
    int ao = 0, cs_a = 0, tx_a = 0;  // patch: slot offset of the next step, its channel step and tap column
    auto fetch_b = [&](f32x4(&b)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b[nt] = buf_ld16(rs_w, wlane + nt * 256u, wp);
        const bool wc = cs_b + 1 == ncs;
        cs_b = wc ? 0 : cs_b + 1;
        wp += w_cs + (wc ? w_dtap : 0);
    };
    auto fetch_a = [&](const f32x4* buf, f32x4(&a)[MT]) __attribute__((always_inline)) {
        const f32x4* qa = buf + ao;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = qa[apix[mt]];
        const bool wc = cs_a + 1 == ncs;
        const bool wx = wc && tx_a + 1 == tap_kw;
        cs_a = wc ? 0 : cs_a + 1;
        tx_a = wx ? 0 : tx_a + (wc ? 1 : 0);
        ao += a_cs + (wc ? a_dtap : 0) + (wx ? a_drow : 0);
    };
    auto first_b = [&](int c0) __attribute__((always_inline)) {
        wp = (c0 >> 2) * cout_slots;
        cs_b = 0;
        fetch_b(b0);
    };
    auto fma_step = [&](const f32x4(&a)[MT], const f32x4(&b)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(a[mt][s], b[nt][s], acc[mt][nt]);
    };

    // ---- one chunk: steps 0 .. nit - 1 of the staged patch `buf` (b0 holds the first step's weights: first_b); `tail` runs behind the
    //      last weight loads of the chunk, two K steps before its end (one when the chunk has a single step) ----
    auto run_chunk = [&](const f32x4* buf, auto&& tail) __attribute__((always_inline)) {
        ao = 0; cs_a = 0; tx_a = 0;
        fetch_a(buf, a0);
        CONV_FENCE
        int it = 0;
        for (; it + 4 <= nit; it += 2) {  // (leaves 2 or 3 steps)
            fetch_b(b1); fetch_a(buf, a1);
            CONV_FENCE
            fma_step(a0, b0);
            CONV_FENCE
            fetch_b(b0); fetch_a(buf, a0);
            CONV_FENCE
            fma_step(a1, b1);
            CONV_FENCE
        }
        const int rem = nit - it;
        if (rem == 3) {
            fetch_b(b1); fetch_a(buf, a1);
            CONV_FENCE
            fma_step(a0, b0);
            CONV_FENCE
            fetch_b(b0); fetch_a(buf, a0);
            tail();
            CONV_FENCE
            fma_step(a1, b1);
            CONV_FENCE
            fma_step(a0, b0);
        } else if (rem == 2) {
            fetch_b(b1); fetch_a(buf, a1);
            tail();
            CONV_FENCE
            fma_step(a0, b0);
            CONV_FENCE
            fma_step(a1, b1);
        } else {
            tail();
            CONV_FENCE
            fma_step(a0, b0);
        }
        CONV_FENCE
    };

    constexpr bool EARLY = EPI != 0 && MT <= 2;  // epilogue pieces fetched in the last chunk's tail
    ConvEpiPre<MT, NT, EPI == 0 ? 1 : EPI> pre;
    if constexpr (EPI != 0) conv_epilogue_prep<MT, NT, EPI>(p, pre, img, oy0, ox0, wm, n_base, li, g, tile_px);
    auto last_tail = [&]() __attribute__((always_inline)) {
        if constexpr (EARLY) conv_epilogue_fetch<MT, NT, EPI>(pre);
    };

    stage_load(0);
    first_b(0);
    stage_store(lds);
    __syncthreads();
    if constexpr (SINGLE) {
        run_chunk(lds, last_tail);
    } else {
        const int bufsz = ckg * plane;
        int pass = 0;
        for (; pass + 1 < npass; ++pass) {
            run_chunk(lds + (pass & 1) * bufsz, [&]() __attribute__((always_inline)) { stage_load((pass + 1) * ck); });
            first_b((pass + 1) * ck);
            stage_store(lds + ((pass + 1) & 1) * bufsz);
            __syncthreads();
        }
        run_chunk(lds + (pass & 1) * bufsz, last_tail);
    }

    if constexpr (EPI == 0) {
        conv_epilogue<MT, NT, 0>(p, acc, img, oy0, ox0, wm, n_base, li, g, tile_px);
    } else {
        if constexpr (!EARLY) conv_epilogue_fetch<MT, NT, EPI>(pre);
        conv_epilogue_form<MT, NT, EPI>(acc, pre, li, g);
    }
}

// One launch = up to kMaxGroups independent convolutions that share (MT, NT): "horizontal fusion" of the
// HRNet branches / fuse terms so that the small low-resolution convs fill the chip together with the large one.
// FORM / EPI: the body and epilogue forms the host resolved for the launch (i2r_conv_plan.h, direct_form): 0 / 0 = conv_body, the general code.
template <int MT, int NT, int CAP, int PF, int FORM = 0, int EPI = 0>
__global__ __launch_bounds__(256) void conv_igemm_f32(const ConvGroupK grp) {
    extern __shared__ __attribute__((aligned(16))) f32x4 lds[];
    int bid = blockIdx.x, gi = 0, start = 0;
    if (grp.blk_map) {
        // host-chosen dispatch order (longest-processing-time packing over the CUs): members of a group have very
        // different K, and with every workgroup resident from the start the hardware cannot rebalance later
        const int v = __builtin_amdgcn_readfirstlane(grp.blk_map[bid]);  // (uniform: keeps the member's fields and buffer descriptors in SGPRs)
        gi = v >> 24;
        bid = v & 0xFFFFFF;
    } else {
#pragma unroll
        for (int i = 0; i < kMaxGroups - 1; ++i)
            if (i + 1 < grp.n && bid >= grp.blk_end[i]) { gi = i + 1; start = grp.blk_end[i]; }
    }
    if constexpr (FORM == 0)
        conv_body<MT, NT, CAP, PF>(grp.g[gi], bid - start, lds);
    else
        conv_body_forms<MT, NT, CAP, PF, FORM == 1, EPI>(grp.g[gi], bid - start, lds);
}

#ifdef I2R_CONV_KERNELS_ONLY  // (tools/conv_sched.py: the kernels alone, instantiated by the including file)
}  // namespace
#else
template <int NT, int CAP, int PF, int FORM, int EPI>
conv_fn pick_mt(int mt) {
    switch (mt) {
        case 1: return conv_igemm_f32<1, NT, CAP, PF, FORM, EPI>;
        case 2: return conv_igemm_f32<2, NT, CAP, PF, FORM, EPI>;
        case 3: return conv_igemm_f32<3, NT, CAP, PF, FORM, EPI>;
        case 4:  // (kDirectFormMaxMT: four M fragments run the general body only)
            if constexpr (FORM == 0) return conv_igemm_f32<4, NT, CAP, PF, 0, 0>;
    }
    return nullptr;
}

template <int CAP, int PF, int FORM, int EPI>
conv_fn pick_nt(int nt, int mt) {
    switch (nt) {
        case 3: return pick_mt<3, CAP, PF, FORM, EPI>(mt);
        case 4: return pick_mt<4, CAP, PF, FORM, EPI>(mt);
        case 5: return pick_mt<5, CAP, PF, FORM, EPI>(mt);
    }
    return nullptr;
}

template <int FORM, int EPI>
conv_fn pick_variant(int nt, int mt, int cap, int pf) {
    if constexpr (FORM == 0) {
        if (pf == 0) return pick_nt<4, 0, 0, 0>(nt, mt);
    }
    if (pf == 1 && cap == 4) return pick_nt<4, 1, FORM, EPI>(nt, mt);
    if (pf == 1 && cap == 12) return pick_nt<12, 1, FORM, EPI>(nt, mt);
    if (pf == 2 && cap == 4) return pick_nt<4, 2, FORM, EPI>(nt, mt);
    return nullptr;
}

}  // namespace

// staging variant: pf 0 = synchronous staging (any patch size / ck); pf 1|2 = double-buffered chunks for patches of up to
// 256|512 pixels with up to cap (4 or 12) channel groups of prefetch registers.  form 1 | 2 (pf > 0 only): the single-chunk | pipelined
// body with the pinned schedule, with epilogue form epi 0 | 1 | 2; form 0 (epi 0): the general body
void* i2r_pick_conv_f32(int nt, int mt, int cap, int pf, int form, int epi) {
    conv_fn fn = nullptr;
    switch (form * 3 + epi) {
        case 0: fn = pick_variant<0, 0>(nt, mt, cap, pf); break;
        case 3: fn = pick_variant<1, 0>(nt, mt, cap, pf); break;
        case 4: fn = pick_variant<1, 1>(nt, mt, cap, pf); break;
        case 5: fn = pick_variant<1, 2>(nt, mt, cap, pf); break;
        case 6: fn = pick_variant<2, 0>(nt, mt, cap, pf); break;
        case 7: fn = pick_variant<2, 1>(nt, mt, cap, pf); break;
        case 8: fn = pick_variant<2, 2>(nt, mt, cap, pf); break;
    }
    return reinterpret_cast<void*>(fn);
}

// the launch logic of the whole conv family (host only): descriptors -> ConvPlan -> launch, and the entry points
#include "i2r_conv_plan.h"
#endif
