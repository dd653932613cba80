// Host planner of the conv family (internal; included once, by i2r_conv.hip below its kernels).  One launch = one ConvPlan: resolve()
// validates every descriptor once (prepare() / prepare_wino() -> a ConvShape per member), settles what the members must share, fills the
// kernel argument (ConvGroupK) and picks the kernel.  Every entry point calls resolve() and reads the plan; nothing here names a kernel
// template (the pickers of i2r_conv.h do).
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "i2r_conv.h"

namespace {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// reciprocals of the kernels' index decodes: ceil(2^32 / d) for div_m (d == 1 has no 32-bit one), ceil(2^31 / d) for div_r
inline unsigned magic(int d) { return d == 1 ? 0u : (unsigned)(((1ull << 32) + d - 1) / d); }
inline unsigned recip31(int d) { return (unsigned)(((1ull << 31) + d - 1) / d); }

// Tuning switches: ablation bits of the kernels (ConvK::dbg), extra LDS plane slots (banks), 0 = no prefetch, prefetch capacity limit.
// Read from the environment once, in a -DI2R_TUNING build only; the product build has the defaults as compile-time constants.
struct ConvTune { int dbg, plane_pad, pf, cap; };
#ifdef I2R_TUNING
inline const ConvTune& conv_tune() {
    auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
    static const ConvTune t = {env("I2R_CONV_DBG", 0), env("I2R_CONV_PLANE_PAD", 0), env("I2R_CONV_PF", 1), env("I2R_CONV_CAP", 12)};
    return t;
}
#else
constexpr ConvTune conv_tune() { return {0, 0, 1, 12}; }
#endif

// What one descriptor (and the group's mt) determines, whatever the other members of the launch are: the result of prepare()
struct ConvShape {
    int nt, wn, mt;                            // fragment split of the output channels, waves along them, M fragments per wave
    int tile_h, tile_w, tiles_y, tiles_x, n_cblk;
    int tap_kh, tap_kw, ph, pw, plane;         // filter grid; input patch of a tile (pixels) and its LDS plane (16-byte slots)
    int npp, cin_g, g_ch;                      // patch pixels per thread (of 256); channel groups = 16-byte LDS slots per patch pixel, channels in one
    int cap, pf, ck;                           // staging variant and channels per pass: the member's own until resolve() imposes the group's
    unsigned in_bytes, w_bytes, out_bytes;     // tensor sizes for the buffer descriptors of the kernels
    size_t lds;                                // LDS bytes of a workgroup
    long long nblk;                            // workgroups (Winograd: fragments -- resolve() settles the runs)
};

// One launch, as every entry point sees it: the result of resolve()
struct ConvPlan {
    ConvGroupK grp;         // the kernel argument
    int algo, dtype;
    int nt, mt, cap, pf;    // the instantiation (cap, pf: implicit GEMM only)
    bool fused_in; int form;  // Winograd: a member has a fused input; epilogue form (wino_form), 0 otherwise
    int dform, depi;        // fp32 implicit GEMM with pf > 0: body and epilogue form (direct_form), 0 / 0 otherwise
    size_t lds; long long total;  // LDS bytes of a workgroup; workgroups
    int seq[kMaxGroups];    // run length per member (1 for implicit GEMM)
    conv_fn fn;             // null: no such instantiation
};

void copy_desc(const i2r_conv_desc* d, ConvK& k) {
    k = ConvK{};
    k.in = d->in; k.in2 = d->in2; k.w = d->w; k.bias = d->bias; k.res1 = d->res1; k.res2 = d->res2; k.res_post = d->res_post; k.out = d->out;
    k.n_img = d->n_img; k.in_h = d->in_h; k.in_w = d->in_w; k.in_cs = d->in_cs; k.cin = d->cin;
    k.conv_h = d->conv_h; k.conv_w = d->conv_w; k.out_h = d->out_h; k.out_w = d->out_w; k.out_cs = d->out_cs;
    k.cout = d->cout; k.cout_pad = d->cout_pad; k.stride = d->stride; k.iy0 = d->iy0; k.ix0 = d->ix0; k.ntaps = d->ntaps;
    k.out_step = d->out_step; k.out_off_y = d->out_off_y; k.out_off_x = d->out_off_x; k.rep = d->rep; k.relu = d->relu;
    k.dtype = d->dtype; k.in16 = d->in_f16; k.out16 = d->out_f16;
    k.algo = d->algo; k.w_seq = 1; k.dbg = conv_tune().dbg;
    k.f_t1 = d->t1; k.f_t2 = d->t2; k.f_y = d->y; k.f_sh1 = d->t1_shift; k.f_sh2 = d->t2 ? d->t2_shift : 0;
}

constexpr int kWinoMaxSeq = 8;       // longest run of fragments a workgroup takes (i2r_conv_desc.seq)
constexpr int kWinoRunPasses = 6;    // passes a run is filled up to when the library chooses
constexpr int kWinoMinWg = 512;      // ... and the workgroups such a launch keeps (of 1024 resident on 256 CUs)
// row pitch (16-byte slots) of a fragment's patch in LDS, fw Winograd tiles across: odd columns sit at + half; 2 * pitch = 8 / 4 / 2 (mod 16)
// for fw = 8 / 4 / 2, so the 16 tiles of a fragment gather 16 distinct slots modulo 16 for every (row, column) of their 4x4 patches
inline int wino_pitch(int fw) { return fw == 8 ? 20 : (fw == 4 ? 10 : 9); }
// runs of a member: its fragment groups in w_seq's
long long wino_runs(const ConvK& k, int mt) { return (((long long)k.w_nfrag + mt - 1) / mt + k.w_seq - 1) / k.w_seq; }

// Winograd F(2x2, 3x3) member (i2r_conv_wino.hip), after the checks of prepare(): fragment shape, patch layout in LDS, fragment count
int prepare_wino(const i2r_conv_desc* d, int force_mt, ConvShape& s) {
    I2R_CHECK_ARG(d->dtype == 0 && !d->in_f16 && !d->out_f16, "i2r_conv: the Winograd kernels are fp32");
    I2R_CHECK_ARG(d->stride == 1 && d->ntaps == 9 && d->iy0 == -1 && d->ix0 == -1 && d->rep == 1 && d->out_step == 1 && d->out_off_y == 0 &&
                      d->out_off_x == 0 && d->in2 == nullptr,
                  "i2r_conv: algo 1 (Winograd) needs a plain 3x3 stride-1 pad-1 convolution");
    for (int t = 0; t < 9; ++t) I2R_CHECK_ARG(d->dy[t] == t / 3 && d->dx[t] == t % 3, "i2r_conv: algo 1 needs row-major 3x3 taps");
    I2R_CHECK_ARG(d->relu == 0 || d->relu == 1, "i2r_conv: algo 1 has no GELU epilogue");
    I2R_CHECK_ARG((long long)d->n_img * d->in_h * d->in_w * d->in_cs < (1ll << 29) && (long long)d->n_img * d->out_h * d->out_w * d->out_cs < (1ll << 29) &&
                      (long long)16 * d->cin * d->cout_pad < (1ll << 29),
                  "i2r_conv: algo 1 addresses its tensors through buffer descriptors of < 2 GiB");
    I2R_CHECK_ARG(d->conv_h == d->in_h && d->conv_w == d->in_w && d->out_h == d->conv_h && d->out_w == d->conv_w, "i2r_conv: algo 1 geometry");
    if (d->t1) {  // fused input: ReLU((in + up(t1)) + up(t2)) staged in place of `in` and written to y
        I2R_CHECK_ARG(d->y != nullptr, "i2r_conv: a fused input (t1) needs y");
        I2R_CHECK_ARG(d->in_cs == d->cin, "i2r_conv: fused input: y is complete only when the conv reads every channel (cin=%d in_cs=%d)", d->cin, d->in_cs);
        for (int t = 0; t < (d->t2 ? 2 : 1); ++t) {
            const int sh = t ? d->t2_shift : d->t1_shift;
            I2R_CHECK_ARG((sh == 1 || sh == 2) && d->in_h % (1 << sh) == 0 && d->in_w % (1 << sh) == 0,
                          "i2r_conv: fused input: t%d_shift %d must be 1 or 2 and the %dx%d map divisible by the scale", t + 1, sh, d->in_h, d->in_w);
        }
        const void* others[] = {d->in, d->t1, d->t2, d->out, d->res1, d->res2, d->res_post};
        for (const void* o : others) I2R_CHECK_ARG((const void*)d->y != o, "i2r_conv: fused input: y aliases another tensor of the launch");
        I2R_CHECK_ARG(d->t1 != (const float*)d->out && d->t2 != (const float*)d->out, "i2r_conv: out aliases a fused-input term");
    }
    const int nfrag = d->cout_pad / 16;
    s.nt = nfrag % 3 == 0 ? 3 : (nfrag % 4 == 0 ? 4 : 0);
    I2R_CHECK_ARG(s.nt != 0, "i2r_conv: algo 1 needs cout_pad=%d to be a multiple of 48 or 64", d->cout_pad);
    s.mt = force_mt ? force_mt : (d->mt ? d->mt : 1);  // (one fragment per item = 4 waves per SIMD: the measured optimum, and the only form built)
    I2R_CHECK_ARG(s.mt == 1, "i2r_conv: algo 1 takes mt 1 (got %d)", s.mt);
    I2R_CHECK_ARG(d->seq >= 0 && d->seq <= kWinoMaxSeq, "i2r_conv: algo 1 runs 1..%d fragments per workgroup (seq=%d; 0 = choose)", kWinoMaxSeq, d->seq);
    int fw = 0;  // Winograd tiles across a fragment of 16 (64 output pixels): the shape that covers the map with the fewest fragments
    if (d->tile_w) {
        I2R_CHECK_ARG(d->tile_w == 16 || d->tile_w == 8 || d->tile_w == 4, "i2r_conv: algo 1 fragment width %d (16, 8, 4)", d->tile_w);
        fw = d->tile_w / 2;
    } else {
        long long best = -1;
        for (int cand : {8, 4, 2}) {
            const long long n = (long long)cdiv(d->conv_w, 2 * cand) * cdiv(d->conv_h, 32 / cand);
            if (best < 0 || n < best) { best = n; fw = cand; }
        }
    }
    s.tile_w = 2 * fw; s.tile_h = 32 / fw;
    s.tiles_x = cdiv(d->conv_w, s.tile_w); s.tiles_y = cdiv(d->conv_h, s.tile_h);
    s.n_cblk = nfrag / s.nt;
    s.ph = s.tile_h + 2; s.pw = s.tile_w + 2; s.tap_kw = s.tap_kh = 3;
    s.plane = cdiv(s.ph * wino_pitch(fw), 16) * 16;
    s.nblk = (long long)d->n_img * s.tiles_y * s.tiles_x;
    // item decode without integer divisions (div_r): exact for n < 2^20 and d < 2^11
    I2R_CHECK_ARG(s.nblk > 0 && (s.nblk + 8) * s.n_cblk < (1ll << 20) && s.tiles_y * s.tiles_x < 2048 && s.n_cblk < 2048, "i2r_conv: algo 1 grid (%lld fragments)", s.nblk);
    s.lds = i2r_conv_wino_lds(s.nt, s.mt, s.plane);
    return I2R_OK;
}

// ... and what its ConvK has beyond the common part of fill_member() (w_seq and w_band: resolve(), once the run lengths are chosen)
void fill_wino(const i2r_conv_desc* d, const ConvShape& s, ConvK& k) {
    const int fw = s.tile_w / 2;
    k.w_fwlog = fw == 8 ? 3 : (fw == 4 ? 2 : 1);
    k.w_half = fw + 1; k.w_pitch = wino_pitch(fw);
    k.w_rcp = (65536 + k.pw - 1) / k.pw;  // exact for pixel indices < 256 and pw in {6, 10, 18}
    k.in_bytes = (unsigned)((long long)d->n_img * d->in_h * d->in_w * d->in_cs * 4);
    k.w_bytes = (unsigned)((long long)16 * d->cin * d->cout_pad * 4);
    k.out_bytes = (unsigned)((long long)d->n_img * d->out_h * d->out_w * d->out_cs * 4);
    if (d->t1) k.f_bytes1 = (unsigned)((long long)d->n_img * (d->in_h >> d->t1_shift) * (d->in_w >> d->t1_shift) * d->in_cs * 4);
    if (d->t2) k.f_bytes2 = (unsigned)((long long)d->n_img * (d->in_h >> d->t2_shift) * (d->in_w >> d->t2_shift) * d->in_cs * 4);
    k.w_m_cblk = magic(k.n_cblk); k.w_m_img = magic(k.tiles_y * k.tiles_x); k.w_m_tx = magic(k.tiles_x);
    k.ck = 16; k.wn = 1;
    k.w_nfrag = (int)s.nblk;
    k.w_seq = d->seq ? d->seq : 1;  // (seq 0: resolve() chooses, seeing the whole group -- wino_choose_seq)
    // what the kernel would otherwise work out per workgroup or read field by field (ConvK::Wino)
    ConvK::Wino& wk = k.wk;
    wk.out = k.out; wk.res1 = k.res1; wk.bias = k.bias;
    wk.out_bytes = k.out_bytes; wk.bias_bytes = (unsigned)d->cout_pad * 4; wk.conv_h = k.conv_h; wk.conv_w = k.conv_w; wk.out_cs = k.out_cs;
    wk.frags_img = k.tiles_y * k.tiles_x; wk.tiles_x = k.tiles_x; wk.r_img = recip31(wk.frags_img); wk.r_tx = recip31(k.tiles_x);
    wk.in_h = k.in_h; wk.in_w = k.in_w; wk.in_cs = k.in_cs;
    wk.pw = k.pw; wk.pp = k.ph * k.pw; wk.w_rcp = k.w_rcp;
    wk.oy_step = k.tile_h; wk.f_sh1 = k.f_sh1; wk.f_sh2 = k.f_sh2; wk.nfrag = k.w_nfrag;
    const int cin4 = d->cin / 4;
    wk.w_row = 4 * cin4 * d->cout_pad * 16;
    wk.w_inc_j = cin4 * d->cout_pad * 16;
    wk.w_inc_wrap = (4 - 3 * cin4) * d->cout_pad * 16;
    wk.npass = d->cin / 16; wk.bufsz = s.mt * 4 * k.plane; wk.nruns = (k.w_nfrag + s.mt - 1) / s.mt;
    wk.n_cblk = k.n_cblk; wk.r_cblk = recip31(k.n_cblk); wk.w_seq = k.w_seq;
    wk.fwlog = k.w_fwlog; wk.pitch = k.w_pitch; wk.half = k.w_half; wk.plane = k.plane; wk.cout_pad = k.cout_pad; wk.ph = k.ph;
    wk.in_bytes = k.in_bytes; wk.w_bytes = k.w_bytes; wk.in = k.in; wk.w = k.w;
}

// Run lengths of the members of a Winograd launch that leave the choice to the library (i2r_conv_desc.seq == 0).  A run saves the
// set-up of every fragment after its first, but it is also a coarser unit of work: the launch is balanced over 256 CUs by the piece,
// and runs of 12 passes (every member as long as a 192-channel item) measured 6 % SLOWER on the whole model than single fragments,
// runs of up to 6 passes 1 % faster ("runs of fragments").  So only the short items are strung together, up to
// kWinoRunPasses passes -- pairs of 48-channel fragments, up to six one-pass fragments; 64 channels and more run alone -- and a
// launch that had kWinoMinWg workgroups at one fragment per workgroup keeps that many (one that had fewer keeps what it had): below
// that floor the longest run (on a tie: of the member with the most passes per fragment) gives a fragment back.
void wino_choose_seq(ConvK* g, const i2r_conv_desc* const* descs, int n, int mt) {
    auto total = [&]() { long long t = 0; for (int i = 0; i < n; ++i) t += wino_runs(g[i], mt) * g[i].n_cblk; return t; };
    long long at_one = 0;
    for (int i = 0; i < n; ++i) at_one += ((long long)g[i].w_nfrag + mt - 1) / mt * g[i].n_cblk;
    const long long floor_wg = std::min<long long>(at_one, kWinoMinWg);
    for (int i = 0; i < n; ++i)
        if (descs[i]->seq == 0) g[i].w_seq = std::max(1, std::min(kWinoMaxSeq, kWinoRunPasses / (g[i].cin >> 4)));
    while (total() < floor_wg) {
        int pick = -1;
        for (int i = 0; i < n; ++i) {
            if (descs[i]->seq != 0 || g[i].w_seq == 1) continue;
            const int len = g[i].w_seq * (g[i].cin >> 4);
            if (pick < 0 || len > g[pick].w_seq * (g[pick].cin >> 4) || (len == g[pick].w_seq * (g[pick].cin >> 4) && g[i].cin > g[pick].cin)) pick = i;
        }
        if (pick < 0) break;  // (only forced members are left)
        --g[pick].w_seq;
    }
}

// Channels per pass and LDS bytes of an implicit-GEMM member under a staging variant -- pf 0: synchronous staging (any patch, any ck);
// pf 1 | 2: double-buffered chunks for patches of up to 256 | 512 pixels, up to `cap` channel groups of prefetch registers each.
// prepare() asks for the member's own variant, resolve() again for the group's where that is another one.
int staging(const i2r_conv_desc* d, int cap, int pf, ConvShape& s) {
    int ckg = 4;  // channel groups per pass
    if (pf > 0) {
        for (int cand : {12, 8, 4})
            if (cand <= cap && s.cin_g % cand == 0 && (size_t)2 * cand * s.plane * 16 <= 40 * 1024) { ckg = cand; break; }
        s.lds = (size_t)2 * ckg * s.plane * 16;
    } else if (d->dtype != 0) {
        // bf16/f16 body: LDS slots hold 8 channels; stage whole 32-channel steps, <= ~24 KB per pass
        const int fit = std::max(4, (24 * 1024 / (s.plane * 16)) / 4 * 4);
        ckg = cdiv(cdiv(s.cin_g, cdiv(s.cin_g, fit)), 4) * 4;
        s.lds = (size_t)ckg * s.plane * 16;
    } else {
        int ck = d->ck;
        if (ck == 0) {
            // small LDS footprint (<= ~20 KB) keeps >= 4 workgroups per CU resident; equal-sized chunks avoid a short tail pass
            int fit = (20 * 1024 / (s.plane * 16)) * 4;
            fit = fit < 16 ? 16 : fit / 16 * 16;
            ck = cdiv(cdiv(d->cin, cdiv(d->cin, fit)), 16) * 16;
        }
        I2R_CHECK_ARG(ck % 16 == 0 && ck >= 16, "i2r_conv: ck=%d", ck);
        ckg = ck / 4;
        s.lds = (size_t)ckg * s.plane * 16;
    }
    s.cap = cap; s.pf = pf; s.ck = ckg * s.g_ch;
    I2R_CHECK_ARG(s.lds <= 160 * 1024, "i2r_conv: LDS %zu B", s.lds);
    return I2R_OK;
}

// Step (a): validate one descriptor and derive what it alone (with the group's mt: force_mt, 0 = free) determines
int prepare(const i2r_conv_desc* d, int force_mt, ConvShape& s) {
    I2R_CHECK_ARG(d && d->in && d->w && d->bias && d->out, "i2r_conv: null pointer");
    I2R_CHECK_ARG(d->cin > 0 && d->cin % 16 == 0 && d->cin <= d->in_cs && d->in_cs % 4 == 0,
                  "i2r_conv: cin=%d must be a multiple of 16 and <= in_cs=%d (in_cs %% 4 == 0)", d->cin, d->in_cs);
    I2R_CHECK_ARG(d->cout > 0 && d->cout_pad % 16 == 0 && d->cout <= d->cout_pad && d->cout <= d->out_cs && d->out_cs % 4 == 0,
                  "i2r_conv: cout=%d cout_pad=%d out_cs=%d", d->cout, d->cout_pad, d->out_cs);
    I2R_CHECK_ARG(d->stride == 1 || d->stride == 2, "i2r_conv: stride %d", d->stride);
    I2R_CHECK_ARG(d->dtype >= 0 && d->dtype <= 2 && (d->dtype == 0 || d->in2 == nullptr), "i2r_conv: dtype %d", d->dtype);
    I2R_CHECK_ARG((d->in_f16 == 0 || d->in_f16 == 1) && (d->out_f16 == 0 || d->out_f16 == 1) && (d->dtype != 0 || (!d->in_f16 && !d->out_f16)),
                  "i2r_conv: 16-bit activation storage (in_f16=%d out_f16=%d) needs a 16-bit operand type (dtype=%d)", d->in_f16, d->out_f16, d->dtype);
    I2R_CHECK_ARG(!d->in_f16 || d->in_cs % 8 == 0, "i2r_conv: 16-bit input needs in_cs %% 8 == 0 (in_cs=%d)", d->in_cs);
    I2R_CHECK_ARG(d->ntaps >= 1 && d->ntaps <= I2R_MAX_TAPS, "i2r_conv: ntaps %d", d->ntaps);
    I2R_CHECK_ARG(d->rep >= 1 && d->out_step >= 1, "i2r_conv: rep/out_step");
    I2R_CHECK_ARG((d->conv_h - 1) * d->out_step + d->out_off_y + d->rep <= d->out_h &&
                      (d->conv_w - 1) * d->out_step + d->out_off_x + d->rep <= d->out_w,
                  "i2r_conv: destination grid exceeds out tensor");
    I2R_CHECK_ARG(d->in2 != (const float*)d->out && d->in != (const float*)d->out, "i2r_conv: out aliases in");
    I2R_CHECK_ARG(d->algo == 0 || d->algo == 1, "i2r_conv: algo %d", d->algo);
    I2R_CHECK_ARG(d->t1 ? d->algo == 1 : (!d->t2 && !d->y), "i2r_conv: a fused input (t1, t2, y) needs algo 1 and starts with t1");
    s = ConvShape{};
    if (d->algo == 1) return prepare_wino(d, force_mt, s);

    int max_dy = 0, max_dx = 0;
    for (int t = 0; t < d->ntaps; ++t) {
        I2R_CHECK_ARG(d->dy[t] >= 0 && d->dx[t] >= 0, "i2r_conv: negative tap offset");
        max_dy = std::max(max_dy, (int)d->dy[t]); max_dx = std::max(max_dx, (int)d->dx[t]);
    }

    // ---- fragment decomposition of the output channels ----
    const int nfrag = d->cout_pad / 16;
    for (int cand : {3, 4, 5})
        if (nfrag % cand == 0) { s.nt = cand; break; }
    I2R_CHECK_ARG(s.nt != 0, "i2r_conv: cout_pad=%d is not a multiple of 48, 64 or 80", d->cout_pad);
    int wn = d->wn;
    if (wn == 0) {
        const int nb = nfrag / s.nt;
        wn = (nb % 4 == 0) ? 4 : (nb % 2 == 0) ? 2 : 1;
        // small-channel layers prefer more pixels per workgroup; keep wn <= 2 unless cout is wide
        if (wn == 4 && d->cout_pad < 192) wn = 2;
    }
    I2R_CHECK_ARG((wn == 1 || wn == 2 || wn == 4) && (nfrag / s.nt) % wn == 0, "i2r_conv: wn=%d does not divide cout", wn);
    const int wm = 4 / wn;

    // ---- tile ----
    int th = d->tile_h, tw = d->tile_w, mt = force_mt ? force_mt : d->mt;
    if (th == 0 || tw == 0) {
        tw = d->conv_w <= 16 ? d->conv_w : (d->conv_w % 16 == 0 ? 16 : (d->conv_w % 12 == 0 ? 12 : 8));
        if (mt == 0) mt = 2;
        th = (wm * mt * 16) / tw;
        th = std::min(std::max(th, 1), d->conv_h);
    }
    if (mt == 0) mt = cdiv(th * tw, wm * 16);
    I2R_CHECK_ARG(mt >= 1 && mt <= 4 && th * tw <= wm * mt * 16, "i2r_conv: tile %dx%d does not fit wm=%d mt=%d", th, tw, wm, mt);
    s.wn = wn; s.mt = mt; s.tile_h = th; s.tile_w = tw;
    s.tiles_y = cdiv(d->conv_h, th); s.tiles_x = cdiv(d->conv_w, tw);
    s.n_cblk = nfrag / (s.nt * wn);
    s.ph = (th - 1) * d->stride + max_dy + 1; s.pw = (tw - 1) * d->stride + max_dx + 1;
    I2R_CHECK_ARG(s.ph * s.pw <= kMaxPP * 256, "i2r_conv: patch %dx%d too large", s.ph, s.pw);
    s.plane = cdiv(s.ph * s.pw, 16) * 16 + conv_tune().plane_pad;
    s.tap_kw = max_dx + 1; s.tap_kh = max_dy + 1;
    for (int t = 0; t < d->ntaps; ++t)
        I2R_CHECK_ARG(d->dy[t] == t / s.tap_kw && d->dx[t] == t % s.tap_kw && d->ntaps == (max_dy + 1) * (max_dx + 1),
                      "i2r_conv: taps must form a dense row-major kh x kw grid");
    // channel groups: 4 fp32 channels, or 8 16-bit channels padded to whole 32-channel MFMA steps
    s.cin_g = d->dtype == 0 ? d->cin / 4 : (d->cin / 8 + 3) / 4 * 4;
    s.g_ch = d->dtype == 0 ? 4 : 8;
    // the member's own staging variant: double-buffered chunks when the patch fits 1-2 pixels per thread (the common case), with the
    // wide prefetch registers (fp32 up to 12 groups, 16-bit up to 8) when a chunk of more than 4 groups divides cin and fits the LDS
    s.npp = cdiv(s.ph * s.pw, 256);
    const int pf = (conv_tune().pf && d->ck == 0 && s.npp <= 2 && s.cin_g % 4 == 0) ? s.npp : 0;
    if (int rc = staging(d, pf == 1 ? std::min(conv_tune().cap, d->dtype == 0 ? 12 : 8) : 4, pf, s)) return rc;
    if (s.ck == 4 * s.g_ch) s.cap = 4;  // (no wider chunk: the kernel with 4 groups of prefetch registers)
    // buffer descriptors of the kernels (in / weights / out): every tensor stays below 2 GiB so that kOOB lies beyond all of them
    const long long esz_in = d->in_f16 ? 2 : 4, esz_out = d->out_f16 ? 2 : 4;
    const long long inb = (long long)d->n_img * d->in_h * d->in_w * d->in_cs * esz_in, outb = (long long)d->n_img * d->out_h * d->out_w * d->out_cs * esz_out;
    const long long wb = d->dtype == 0 ? (long long)d->ntaps * d->cin * d->cout_pad * 4 : (long long)d->ntaps * s.cin_g * 8 * d->cout_pad * 2;
    I2R_CHECK_ARG(inb < (1ll << 31) && outb < (1ll << 31) && wb < (1ll << 31), "i2r_conv: tensors of 2 GiB and more are not supported (in %lld, out %lld, weights %lld bytes)", inb, outb, wb);
    s.in_bytes = (unsigned)inb; s.out_bytes = (unsigned)outb; s.w_bytes = (unsigned)wb;
    s.nblk = (long long)d->n_img * s.tiles_y * s.tiles_x * s.n_cblk;
    I2R_CHECK_ARG(s.nblk > 0 && s.nblk < (1ll << 30), "i2r_conv: grid");
    // ranges of the reciprocal divisions in the kernels (div_m): n < 2^32 / d
    I2R_CHECK_ARG(s.nblk * std::max(s.n_cblk, std::max(s.tiles_x, s.tiles_y)) < (1ll << 32) && (long long)kMaxPP * 256 * s.pw < (1ll << 32),
                  "i2r_conv: grid of %lld workgroups exceeds the index-decode range", s.nblk);
    return I2R_OK;
}

// Step (b): the ConvK of a member (either algorithm) whose shape and staging variant are settled
void fill_member(const i2r_conv_desc* d, const ConvShape& s, ConvK& k) {
    copy_desc(d, k);
    k.tile_h = s.tile_h; k.tile_w = s.tile_w; k.tiles_y = s.tiles_y; k.tiles_x = s.tiles_x; k.n_cblk = s.n_cblk;
    k.ph = s.ph; k.pw = s.pw; k.plane = s.plane; k.tap_kw = s.tap_kw; k.tap_kh = s.tap_kh;
    if (d->algo == 1) return fill_wino(d, s, k);
    k.ck = s.ck; k.wn = s.wn;
    k.in_bytes = s.in_bytes; k.out_bytes = s.out_bytes; k.w_bytes = s.w_bytes;
    k.m_cblk = magic(k.n_cblk); k.m_tx = magic(k.tiles_x); k.m_ty = magic(k.tiles_y); k.m_pw = magic(k.pw); k.m_tw = magic(k.tile_w);
    k.wn_log = s.wn == 4 ? 2 : (s.wn == 2 ? 1 : 0);
    k.npass = s.cin_g / (s.ck / s.g_ch);  // chunks per workgroup (the double-buffered variants use it)
}

// a grouped Winograd launch takes the fused-input form of the kernel only when a member needs it
bool any_fused_input(const i2r_conv_desc* const* descs, int32_t n) {
    return std::any_of(descs, descs + n, [](const i2r_conv_desc* d) { return d->t1 != nullptr; });
}

// Epilogue form of a Winograd launch (conv_wino_body's EPI): the two shapes of the HRNet tower -- bias + ReLU (1), bias + res1 + ReLU
// (2) -- are compiled without flag tests and taken when EVERY member has that shape: ReLU, no res2 / res_post, channel blocks exact in
// cout and out_cs (no tail), and all members with or all without res1.  Everything else, a tuning build with ablation bits, and every
// launch while the switch below is off run the general form 0.  The results do not depend on the form, bit for bit.
std::atomic<int> g_wino_forms{1};

int wino_form(const i2r_conv_desc* const* descs, int32_t n, const ConvGroupK& grp) {
    if (!g_wino_forms.load(std::memory_order_relaxed)) return 0;
    for (int i = 0; i < n; ++i) {
        const i2r_conv_desc* d = descs[i];
        if (d->relu != 1 || d->res2 || d->res_post || d->cout != d->cout_pad || d->cout_pad > d->out_cs) return 0;
        if ((d->res1 != nullptr) != (descs[0]->res1 != nullptr)) return 0;
        if (I2R_DBG(grp.g[i]) != 0) return 0;
    }
    return descs[0]->res1 ? 2 : 1;
}

// Body and epilogue form of an fp32 implicit-GEMM launch of a double-buffered variant (conv_igemm_f32's FORM / EPI, i2r_conv.hip).
// Body: 1 when every member has a single channel chunk, else 2 (which also runs one-chunk members).  Epilogue: the rule of wino_form,
// and every pixel written once (rep 1; out_step / offsets are free: the deconv parities qualify).  The synchronous variant (pf 0), a tuning
// build with ablation bits (the stamps and switches live in the general body), a member with a second input (in2), four M fragments per wave (no launch of the models has
// them; the forms are not compiled for it) and every launch while the switch is off: 0 / 0.
std::atomic<int> g_direct_forms{1};
constexpr int kDirectFormMaxMT = 3;

void direct_form(const i2r_conv_desc* const* descs, int32_t n, const ConvGroupK& grp, int pf, int mt, int& form, int& epi) {
    form = epi = 0;
    if (pf == 0 || mt > kDirectFormMaxMT || descs[0]->algo != 0 || descs[0]->dtype != 0 || !g_direct_forms.load(std::memory_order_relaxed)) return;
    for (int i = 0; i < n; ++i)
        if (I2R_DBG(grp.g[i]) != 0 || descs[i]->in2) return;  // (in2: conv_body's order, see conv_body_forms)
    form = 1;
    epi = descs[0]->res1 ? 2 : 1;
    for (int i = 0; i < n; ++i) {
        const i2r_conv_desc* d = descs[i];
        if (grp.g[i].npass != 1) form = 2;
        if (d->relu != 1 || d->res2 || d->res_post || d->rep != 1 || d->cout != d->cout_pad || d->cout_pad > d->out_cs ||
            (d->res1 != nullptr) != (descs[0]->res1 != nullptr))
            epi = 0;
    }
}

// The plan of a launch.  with_table: the launch has a dispatch table (i2r_conv_grouped's block_map); without one a Winograd launch
// numbers its items in XCD bands, which changes its grid.
int resolve(const i2r_conv_desc* const* descs, int32_t n, bool with_table, ConvPlan& p) {
    I2R_CHECK_ARG(descs && n >= 1 && n <= kMaxGroups, "i2r_conv_grouped: 1..%d descriptors", kMaxGroups);
    for (int i = 0; i < n; ++i) I2R_CHECK_ARG(descs[i] && descs[i]->algo == descs[0]->algo, "i2r_conv_grouped: members mix algorithms");
    ConvShape sh[kMaxGroups];
    ConvGroupK& grp = p.grp;
    // what the members of a launch must share; members after the first are shaped with the first member's mt
    auto agrees = [&](int i) -> int {
        I2R_CHECK_ARG(sh[i].nt == sh[0].nt && sh[i].mt == sh[0].mt, "i2r_conv_grouped: descriptor %d has fragment blocking (%d,%d) != (%d,%d)", i,
                      sh[i].mt, sh[i].nt, sh[0].mt, sh[0].nt);
        I2R_CHECK_ARG(descs[i]->dtype == descs[0]->dtype, "i2r_conv_grouped: members mix compute dtypes");
        return I2R_OK;
    };
    // an implicit-GEMM group settles on one staging variant once every member is known; all other launches are checked member by member
    const bool settle = n > 1 && descs[0]->algo == 0;
    for (int i = 0; i < n; ++i) {
        int rc = prepare(descs[i], i ? sh[0].mt : 0, sh[i]);
        if (!rc && !settle) rc = agrees(i);
        if (rc) return rc;
    }
    if (settle) {
        // the most general variant any member needs: pf 0 if one needs it, else the largest pf; the largest cap only among pf 1
        int pf = 0, cap = 4;
        bool all_pf = true;
        for (int i = 0; i < n; ++i) {
            all_pf = all_pf && sh[i].pf != 0;
            pf = std::max(pf, sh[i].pf);
            cap = std::max(cap, sh[i].cap);
        }
        if (!all_pf) pf = 0;
        if (pf != 1) cap = 4;
        for (int i = 0; i < n; ++i) {
            int rc = (sh[i].cap != cap || sh[i].pf != pf) ? staging(descs[i], cap, pf, sh[i]) : I2R_OK;
            if (!rc) rc = agrees(i);
            if (rc) return rc;
        }
    }
    p.algo = descs[0]->algo; p.dtype = descs[0]->dtype;
    p.nt = sh[0].nt; p.mt = sh[0].mt; p.cap = sh[0].cap; p.pf = sh[0].pf;
    p.lds = 0; p.total = 0;
    for (int i = 0; i < n; ++i) fill_member(descs[i], sh[i], grp.g[i]);
    if (p.algo == 1) wino_choose_seq(grp.g, descs, n, p.mt);
    for (int i = 0; i < n; ++i) {
        ConvK& k = grp.g[i];
        long long nblk = sh[i].nblk;
        if (p.algo == 1) {
            const long long runs = wino_runs(k, p.mt);
            nblk = runs * k.n_cblk;
            if (!with_table) {  // XCD-aware item numbering of the Winograd kernels (i2r_conv_wino.hip): whole rounds of 8 runs
                k.w_band = (int)((runs + 7) / 8);
                nblk = (long long)k.w_band * 8 * k.n_cblk;
            }
            k.wk.w_seq = k.w_seq; k.wk.w_band = k.w_band;
        }
        p.lds = std::max(p.lds, sh[i].lds);
        p.total += nblk;
        grp.blk_end[i] = (int)p.total;
        p.seq[i] = k.w_seq;
    }
    for (int i = n; i < kMaxGroups; ++i) { grp.g[i] = grp.g[0]; grp.blk_end[i] = (int)p.total; p.seq[i] = 0; }
    grp.n = n; grp.blk_map = nullptr;
    I2R_CHECK_ARG(p.total < (1ll << 31), "i2r_conv_grouped: grid");
    p.fused_in = p.algo == 1 && any_fused_input(descs, n);
    p.form = p.algo == 1 ? wino_form(descs, n, grp) : 0;
    direct_form(descs, n, grp, p.pf, p.mt, p.dform, p.depi);
    p.fn = reinterpret_cast<conv_fn>(p.algo == 1    ? i2r_pick_conv_wino(p.nt, p.mt, p.fused_in, p.form)
                                     : p.dtype == 0 ? i2r_pick_conv_f32(p.nt, p.mt, p.cap, p.pf, p.dform, p.depi)
                                     : p.dtype == 1 ? i2r_pick_conv_bf16(p.nt, p.mt, p.cap, p.pf)
                                                    : i2r_pick_conv_f16(p.nt, p.mt, p.cap, p.pf));
    return I2R_OK;
}

}  // namespace

extern "C" int i2r_conv_wino_forms(int32_t on) {
    g_wino_forms.store(on ? 1 : 0, std::memory_order_relaxed);
    return I2R_OK;
}

extern "C" int i2r_conv_wino_form(const i2r_conv_desc* const* descs, int32_t n, int32_t* form) {
    ConvPlan p;
    if (int rc = resolve(descs, n, true, p)) return rc;
    I2R_CHECK_ARG(form != nullptr, "i2r_conv_wino_form: form");
    *form = p.form;
    return I2R_OK;
}

extern "C" int i2r_conv_direct_forms(int32_t on) {
    g_direct_forms.store(on ? 1 : 0, std::memory_order_relaxed);
    return I2R_OK;
}

extern "C" int i2r_conv_direct_form(const i2r_conv_desc* const* descs, int32_t n, int32_t* form, int32_t* epi) {
    ConvPlan p;
    if (int rc = resolve(descs, n, true, p)) return rc;
    I2R_CHECK_ARG(form != nullptr, "i2r_conv_direct_form: form");
    *form = p.dform;
    if (epi) *epi = p.depi;
    return I2R_OK;
}

extern "C" int i2r_conv_grouped(const i2r_conv_desc* const* descs, int32_t n, const int32_t* block_map, int32_t map_len, void* stream) {
    ConvPlan p;
    if (int rc = resolve(descs, n, block_map != nullptr, p)) return rc;
    p.grp.blk_map = block_map;
    I2R_CHECK_ARG(block_map == nullptr || map_len == (int32_t)p.total, "i2r_conv_grouped: block_map has %d entries, grid has %lld", map_len, p.total);
    I2R_CHECK_ARG(p.fn != nullptr, "i2r_conv: no kernel for nt=%d mt=%d cap=%d pf=%d dtype=%d", p.nt, p.mt, p.cap, p.pf, p.dtype);
    if (p.lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(p.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
    i2r_launch(p.fn, dim3((unsigned)p.total), dim3(256), p.lds, (hipStream_t)stream, p.grp);
    I2R_CHECK_LAUNCH("i2r_conv");
    return I2R_OK;
}

extern "C" int i2r_conv(const i2r_conv_desc* d, void* stream) { return i2r_conv_grouped(&d, 1, nullptr, 0, stream); }

extern "C" int i2r_conv_grid(const i2r_conv_desc* const* descs, int32_t n, int32_t with_map, int32_t* grid, int32_t* seq) {
    ConvPlan p;
    if (int rc = resolve(descs, n, with_map != 0, p)) return rc;
    I2R_CHECK_ARG(grid != nullptr, "i2r_conv_grid: grid");
    *grid = (int32_t)p.total;
    if (seq) std::copy(p.seq, p.seq + n, seq);
    return I2R_OK;
}

extern "C" int i2r_conv_kernel_name(const i2r_conv_desc* const* descs, int32_t n, char* buf, int32_t buflen) {
    ConvPlan p;
    if (int rc = resolve(descs, n, true, p)) return rc;
    I2R_CHECK_ARG(buf && buflen > 0, "i2r_conv_kernel_name: buffer");
    if (p.algo == 1)
        snprintf(buf, (size_t)buflen, "conv_wino_%sf32<%d, %d>", p.fused_in ? "fin_" : "", p.mt, p.nt);
    else if (p.dtype)
        snprintf(buf, (size_t)buflen, "conv_igemm_lp<%d, %d, %d, %d>/%s", p.mt, p.nt, p.cap, p.pf, p.dtype == 1 ? "bf16" : "f16");
    else
        snprintf(buf, (size_t)buflen, "conv_igemm_f32<%d, %d, %d, %d>", p.mt, p.nt, p.cap, p.pf);
    return I2R_OK;
}
