// The TN kernel of the split-precision (f16x3) GEMMs - weight gradients: the kernel, its split rule and launch plan, the launcher and
// the op-level wrapper.  Representation, scale rule and plane layout: xv_gemm16.h.
//
// P[split][m][n] = (sum_r A[amap(r)][m] * B[bmap(r)][n]) / (sA*sB)
// LDS image per plane: [32 reduction rows][128 columns] fp16, exactly as in HBM (LDS-DMA, no transpose).  The MFMA
// wants 8 consecutive r per lane at a fixed column - a column read: ds_read_b64_tr_b16 delivers a 4-row x 16-column
// block transposed (lane t of a 16-lane group gets column t of the 4 rows); two of them form one operand.
// Rows are 256 B = one full bank row apart, so the 32-byte column blocks are XOR-swizzled by the row
// (block ^= 2*(row&3)) on the DMA source address and on the read address: conflict-free.
#include "xv_gemm16.h"

struct TN16Args {
    const u16* A; long lda; long a_plane; int a_pitch;
    const u16* B; long ldb; long b_plane; int b_pitch;
    int rps; float inv_rps;
    float* P;
    int M, N, R, r_chunk;
    int tiles_m, tiles_n;
    const unsigned* a_amax; const unsigned* b_amax;
    const u16* zero;
};

#define TN16_BR 32      // reduction rows per stage

__global__ __launch_bounds__(256, 2) void xv_gemm16_tn_kernel(TN16Args p) {
    constexpr int BR = TN16_BR;
    constexpr int PH = BR * 128;                  // halfs per plane image
    constexpr int BH = 4 * PH;                    // per buffer: A planes, B planes
    __shared__ __attribute__((aligned(16))) u16 smem[2 * BH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int wr = wave >> 1, wc = wave & 1;
    const int v = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tiles = p.tiles_m * p.tiles_n;
    const int split = v / tiles, t = v - split * tiles;
    const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int r_begin = split * p.r_chunk;
    const int r_end = min(p.R, r_begin + p.r_chunk);
    const int nk = (r_end - r_begin + BR - 1) / BR;

    // DMA: one wave-instruction = 4 image rows x 256 B; lane -> row l>>4, 16-byte chunk position l&15
    const int drow = lane >> 4, dpos = lane & 15;
    // 16x16x32: the four 16-lane groups of a transposed read sit on rows 8g + {0..3} (+4) of one 32-byte column block; the block
    // position is XOR-ed with 2*(row&3) ^ ((row>>3)&1) so that the 8 (group, row) pairs of each half-wave take 8 distinct blocks
    const int scol = (((((dpos >> 1) ^ (2 * drow) ^ (wave & 1)) << 1) | (dpos & 1))) * 8;    // rows 8*wave + 4*i + drow: (row>>3)&1 = wave&1
    const bool a_cv = (m0 + scol) < p.M, b_cv = (n0 + scol) < p.N;
    auto gstage_ragged = [&](int kt, int buf) {      // a stage with rows at or beyond r_end: those read the zero page (they are summed)
        u16* base = smem + buf * BH;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rg = 2 * uwave + i;                     // image rows 4*rg .. 4*rg+3
            int r = r_begin + kt * BR + 4 * (2 * wave + i) + drow;
            bool rv = r < r_end;
            int seg = (int)((float)r * p.inv_rps);            // r / rps without an integer divide (r < 2^24)
            int tt = r - seg * p.rps;
            seg += (tt >= p.rps) - (tt < 0);
            tt = r - seg * p.rps;
            const long ao = ((long)seg * p.a_pitch + tt) * p.lda + m0 + scol;
            const long bo = ((long)seg * p.b_pitch + tt) * p.ldb + n0 + scol;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const u16* pa = (rv && a_cv) ? p.A + pl * p.a_plane + ao : p.zero;
                const u16* pb = (rv && b_cv) ? p.B + pl * p.b_plane + bo : p.zero;
                xv_dma16_ptr(pa, base + pl * PH + 4 * rg * 128);
                xv_dma16_ptr(pb, base + (2 + pl) * PH + 4 * rg * 128);
            }
        }
    };
    // Full stages: scalar plane bases + 32-bit lane offsets that advance by BR rows per stage (xv_dma16; the fp32 weight-gradient kernel's
    // scheme, xv_gemm_tn.hip): a row of the spliced view is (segment, frame), frame += BR, and on crossing a segment's last frame the offset
    // skips the rows between two segments.  Columns outside the matrix read column 0: their products are never stored.
    const bool steady = p.rps >= BR;
    int tt_i[2];
    unsigned aoff[2], boff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = min(r_begin + 4 * (2 * wave + i) + drow, p.R - 1);
        const int seg = r / p.rps;
        tt_i[i] = r - seg * p.rps;
        aoff[i] = (unsigned)((((long)seg * p.a_pitch + tt_i[i]) * p.lda + (a_cv ? m0 + scol : 0)) * 2);
        boff[i] = (unsigned)((((long)seg * p.b_pitch + tt_i[i]) * p.ldb + (b_cv ? n0 + scol : 0)) * 2);
    }
    const unsigned a_step = (unsigned)(BR * p.lda * 2), b_step = (unsigned)(BR * p.ldb * 2);
    const unsigned a_skip = (unsigned)((long)(p.a_pitch - p.rps) * p.lda * 2), b_skip = (unsigned)((long)(p.b_pitch - p.rps) * p.ldb * 2);
    const unsigned lds0 = xv_lds_addr(smem + 4 * 2 * uwave * 128);
    auto gstage = [&](int kt, int buf) {
        if (!steady || r_begin + (kt + 1) * BR > r_end) {
            gstage_ragged(kt, buf);
            return;
        }
        // (kt counts up by one per call, so the offsets are at stage kt here)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                xv_dma16((const float*)(p.A + pl * p.a_plane), aoff[i], lds0 + (buf * BH + pl * PH + 4 * i * 128) * 2);
                xv_dma16((const float*)(p.B + pl * p.b_plane), boff[i], lds0 + (buf * BH + (2 + pl) * PH + 4 * i * 128) * 2);
            }
            tt_i[i] += BR;
            const bool wrap = tt_i[i] >= p.rps;
            tt_i[i] -= wrap ? p.rps : 0;
            aoff[i] += a_step + (wrap ? a_skip : 0u);
            boff[i] += b_step + (wrap ? b_skip : 0u);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // transposed-read lane geometry: 16-lane group lg = lane>>4 = k group (rows 8*lg .. 8*lg+7 of the stage), the 16 lanes of a group
    // cover 4 rows x 16 columns (lane t ends up with column t of the 4 rows)
    const int lc = lane & 15, lg = lane >> 4;
    const int tq = lc >> 2, tp = lc & 3;
    auto tr_off = [&](int cb /* 16-column block 0..7 */, int rbase /* 0 | 4 */) {
        const int r = 8 * lg + rbase + tq;
        return r * 128 + ((cb ^ (2 * (r & 3)) ^ ((r >> 3) & 1)) << 4) + tp * 4;
    };
    typedef __attribute__((address_space(3))) s16x4* ltr_t;
    if (nk > 0) gstage(0, 0);
    xv16_sync();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gstage(kt + 1, buf ^ 1);
        const u16* base = smem + buf * BH;
        s16x8 af[2][4], bf[2][4];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const u16* ia = base + pl * PH;
                const u16* ib = base + (2 + pl) * PH;
                s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(ia + tr_off(4 * wr + qd, 0)));
                s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(ia + tr_off(4 * wr + qd, 4)));
                s16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(ib + tr_off(4 * wc + qd, 0)));
                s16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ltr_t)(ib + tr_off(4 * wc + qd, 4)));
                af[pl][qd] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
                bf[pl][qd] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) XV16_MFMA3_16X16X32(acc[a][b], af, bf, a, b);
        xv16_sync();
    }
    const float out_scale = 1.0f / (xv_pow2_scale(p.a_amax ? *p.a_amax : 0u) * xv_pow2_scale(p.b_amax ? *p.b_amax : 0u));
    float* P = p.P + (long)split * p.M * p.N;
    // (the block stores are written out here and in the context-window kernel: a shared function changed the streams, profiles/gemm16_split_isa.txt)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = n0 + wc * 64 + b * 16 + lc;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int m = m0 + wr * 64 + a * 16 + lg * 4 + jj;
                if (m < p.M && n < p.N) P[(long)m * p.N + n] = acc[a][b][jj] * out_scale;
            }
        }
}

int xv_tn16_splits(int M, int N, int R) {
    int tiles = xv_cdiv(M, 128) * xv_cdiv(N, 128);
    int ksteps = xv_cdiv(R, TN16_BR);
    int splits = 512 / tiles;                      // 2 resident workgroups per CU (64 KB LDS each): one co-resident round
    if (splits > ksteps / 2) splits = ksteps / 2;
    if (splits < 1) splits = 1;
    int chunk = xv_cdiv(ksteps, splits) * TN16_BR;
    return xv_cdiv(R, chunk);
}

// The launch plan of a TN problem, stated once: xv_launch_gemm16_tn runs it, xv_debug_gemm16_tn_plan reports it.
struct TN16Plan {
    int tiles_m, tiles_n;
    int rps, a_pitch, b_pitch;      // as the kernel sees them: gap-free rows are one segment of R rows
    int collapsed;                  // 1: the rows were gap-free
    int r_chunk;                    // reduction rows per split, a multiple of TN16_BR
    int steady;                     // 1: whole stages advance lane offsets (rps >= TN16_BR); 0: every stage takes the per-row form
};

static int tn16_check_shape(const XvGemm16TN& g) {
    XV_REQUIRE(g.lda % 8 == 0 && g.ldb % 8 == 0 && g.M % 8 == 0 && g.N % 8 == 0, "gemm16_tn: lda/ldb/M/N must be multiples of 8 (M=%d N=%d)", g.M, g.N);
    XV_REQUIRE(g.R > 0 && g.R < (1 << 24) && g.rps > 0 && g.splits >= 1, "gemm16_tn: bad reduction shape");
    {   // xv_dma16 addresses every row of a plane as a 32-bit byte offset from the plane's base
        const long segs = xv_cdiv(g.R, g.rps);
        XV_REQUIRE((segs * g.a_pitch + 1) * g.lda * 2 < (1L << 32) && (segs * g.b_pitch + 1) * g.ldb * 2 < (1L << 32),
                   "gemm16_tn: a plane spans 4 GB or more (%ld segments, lda=%ld ldb=%ld): split the batch", segs, g.lda, g.ldb);
    }
    return 0;
}

static int tn16_plan(const XvGemm16TN& g, TN16Plan* t) {
    t->rps = g.rps; t->a_pitch = g.a_pitch; t->b_pitch = g.b_pitch;
    // gap-free rows (every dense layer: one-frame "segments") are one segment of R rows, so the K-steps take the cheap form (xv_launch_gemm_tn)
    t->collapsed = (g.a_pitch == g.rps && g.b_pitch == g.rps) ? 1 : 0;
    if (t->collapsed) { t->rps = g.R; t->a_pitch = g.R; t->b_pitch = g.R; }
    t->tiles_m = xv_cdiv(g.M, 128); t->tiles_n = xv_cdiv(g.N, 128);
    int ksteps = xv_cdiv(g.R, TN16_BR);
    t->r_chunk = xv_cdiv(ksteps, g.splits) * TN16_BR;
    XV_REQUIRE(xv_cdiv(g.R, t->r_chunk) == g.splits, "gemm16_tn: splits must come from xv_tn16_splits");
    t->steady = t->rps >= TN16_BR ? 1 : 0;
    return 0;
}

extern "C" int xv_debug_gemm16_tn_plan(int M, int N, int R, int rps, int a_pitch, int b_pitch, int out[5]) {
    XV_REQUIRE(out, "xv_debug_gemm16_tn_plan: out is NULL");
    XV_REQUIRE(M > 0 && N > 0, "gemm16_tn: bad reduction shape");
    XvGemm16TN g = {};
    g.M = M; g.N = N; g.R = R; g.rps = rps; g.a_pitch = a_pitch; g.b_pitch = b_pitch; g.lda = M; g.ldb = N;
    g.splits = 1;
    if (int rc = tn16_check_shape(g)) return rc;
    g.splits = xv_tn16_splits(M, N, R);
    TN16Plan t;
    if (int rc = tn16_plan(g, &t)) return rc;
    out[0] = t.tiles_m * t.tiles_n; out[1] = g.splits; out[2] = t.r_chunk; out[3] = t.collapsed; out[4] = t.steady;
    return 0;
}

int xv_launch_gemm16_tn(hipStream_t s, const XvGemm16TN& g) {
    if (int rc = tn16_check_shape(g)) return rc;
    TN16Plan t;
    if (int rc = tn16_plan(g, &t)) return rc;
    TN16Args p;
    p.zero = (const u16*)xv_zero_page();
    if (!p.zero) return 1;
    p.A = (const u16*)g.A; p.lda = g.lda; p.a_plane = g.a_plane; p.a_pitch = t.a_pitch;
    p.B = (const u16*)g.B; p.ldb = g.ldb; p.b_plane = g.b_plane; p.b_pitch = t.b_pitch;
    p.rps = t.rps;
    p.inv_rps = 1.0f / (float)p.rps;
    p.P = g.P; p.M = g.M; p.N = g.N; p.R = g.R;
    p.tiles_m = t.tiles_m; p.tiles_n = t.tiles_n;
    p.r_chunk = t.r_chunk;
    p.a_amax = g.a_amax; p.b_amax = g.b_amax;
    dim3 grid(p.tiles_m * p.tiles_n * g.splits);
    XvProfScope prof(s, 5, 2.0 * g.M * g.N * g.R);
    hipLaunchKernelGGL(xv_gemm16_tn_kernel, grid, dim3(256), 0, s, p);
    XV_LAUNCH_CHECK();
    return 0;
}

// Public op-level wrapper (include/xvector_hip.h, "split precision")
extern "C" int xv_affine_wgrad_f16x3(void* stream, const void* x_planes, size_t x_plane_stride, const uint32_t* x_amax, int segs, int t_in,
                                     int c_ld, int k, int c, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax,
                                     int dz_seg_pitch, int dz_row0, int o_ld, int o, const float* kernel, float l2_scale, float* dkernel,
                                     void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_in >= k && c_ld >= c && o_ld >= o && o_ld % 8 == 0 && c_ld % 8 == 0,
               "affine_wgrad_f16x3: bad shape (c_ld=%d and o_ld=%d must be multiples of 8)", c_ld, o_ld);
    const int t_out = t_in - k + 1;
    XvGemm16TN g = {};
    g.A = x_planes; g.lda = c_ld; g.a_plane = (long)x_plane_stride; g.a_pitch = t_in;
    g.B = (const u16*)dz_planes + (long)dz_row0 * o_ld; g.ldb = o_ld; g.b_plane = (long)dz_plane_stride; g.b_pitch = dz_seg_pitch;
    g.rps = t_out;
    g.M = k * c_ld; g.N = o_ld; g.R = segs * t_out;
    g.splits = xv_tn16_splits(g.M, g.N, g.R);
    XV_REQUIRE((size_t)g.splits * g.M * g.N * sizeof(float) <= ws_bytes, "affine_wgrad_f16x3: workspace too small (%zu needed)",
               (size_t)g.splits * g.M * g.N * sizeof(float));
    g.P = (float*)ws;
    g.a_amax = x_amax; g.b_amax = dz_amax;
    int rc = xv_launch_gemm16_tn((hipStream_t)stream, g);
    if (rc) return rc;
    return xv_launch_wgrad_reduce((hipStream_t)stream, g.P, g.splits, k, c, c_ld, o_ld, o, l2_scale != 0.f ? kernel : nullptr, o, l2_scale,
                                  dkernel, o);
}
