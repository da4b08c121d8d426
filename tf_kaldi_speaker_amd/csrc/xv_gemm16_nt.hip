// The NT kernels of the split-precision (f16x3) GEMMs - forward and data gradient: the generic kernel, the context-window kernel, the
// rule that picks one (nt16_form), the launcher and the op-level wrappers.  Representation, scale rule and plane layout: xv_gemm16.h.
#include "xv_gemm16.h"

// ---------------------------------------------------------------------------------------------
// NT: C[m][n] = (sum_k A[rowmap(m)][k] * Bt[n][k]) / (sA*sB) + bias[n]
// 128x128 tile, 4 waves (2x2) x 64x64 = 2x2 v_mfma_f32_32x32x16_f16 accumulators, K-step 32, two operands x two
// planes x [128][32] fp16 LDS images (64 KB double-buffered, 2 workgroups per CU) filled by LDS-DMA; 16-byte
// chunks XOR-swizzled by (row>>2)&3 on the DMA source and the ds_read_b128 address (conflict-free).
// ---------------------------------------------------------------------------------------------
struct NT16Args {
    const u16* A; long lda; long a_plane; int a_rps; int a_pitch;
    const u16* Bt; long ldb; long b_plane;
    float* C; long ldc;
    int M, N, K;
    int tiles_m, tiles_n;
    const float* bias;
    float* part;
    const unsigned* a_amax; const unsigned* b_amax;
    const u16* zero;
    XvBwdStats bwd;         // EPI == 2 only
};

#define WN16 2                         // waves along N (4 waves: 2x2 of 64x64)
#define NB16 2                         // 32-column accumulator blocks per wave
#define BK16 32                        // halfs per K-step
#define SWZ16(row) (((row) >> 2) & 3)
#define CQ16 (BK16 / 8)
#define PLANE_HALFS (128 * BK16)
#define BUF_HALFS (4 * PLANE_HALFS)

template <int EPI>      // 0: plain, 1: + forward BN statistics of the tile, 2: + BN backward reductions (data gradient)
__global__ __launch_bounds__(256, 2) void xv_gemm16_nt_kernel(NT16Args p) {
    constexpr int RPI = 64 / CQ16;                 // tile rows per LDS-DMA wave-instruction (16)
    constexpr int IPW = 128 / RPI / 4;             // DMA instructions per wave per plane per operand
    __shared__ __attribute__((aligned(16))) u16 smem[2 * BUF_HALFS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int wr = wave / WN16, wc = wave % WN16;
    const int li = lane & 31, lh = lane >> 5;
    const int t = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
    const int m0 = tile_m * 128, n0 = tile_n * 128;
    const int nk = (p.K + BK16 - 1) / BK16;

    const int lrow = lane / CQ16, lpos = lane % CQ16;
    // per-lane byte offsets from the plane bases, swizzled chunk folded in (xv_dma16: scalar base + 32-bit offset, xv_handoff.h; both planes
    // share them).  Rows outside the matrix read row 0 - their products are never stored or counted; k beyond K must read zeros and
    // takes the zero page through the builtin's 64-bit form (a ragged last K-step only).
    unsigned aoff[IPW], boff[IPW];
    int ksrc[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int row = RPI * (IPW * wave + i) + lrow;
        ksrc[i] = ((lpos ^ SWZ16(row)) << 3);
        int m = m0 + row;
        int mm = m < p.M ? m : 0;
        int seg = mm / p.a_rps, tt = mm - seg * p.a_rps;
        aoff[i] = (unsigned)((((long)seg * p.a_pitch + tt) * p.lda + ksrc[i]) * 2);
        int n = n0 + row;
        boff[i] = (unsigned)(((long)(n < p.N ? n : 0) * p.ldb + ksrc[i]) * 2);
    }
    const unsigned lds0 = xv_lds_addr(smem + RPI * IPW * uwave * BK16);
    auto gstage = [&](int kt, int buf) {
        const int k0 = kt * BK16;
        if (k0 + BK16 <= p.K) {
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const float* abase = (const float*)(p.A + pl * p.a_plane + k0);
                const float* bbase = (const float*)(p.Bt + pl * p.b_plane + k0);
#pragma unroll
                for (int i = 0; i < IPW; ++i) {
                    xv_dma16(abase, aoff[i], lds0 + (buf * BUF_HALFS + pl * PLANE_HALFS + RPI * i * BK16) * 2);
                    xv_dma16(bbase, boff[i], lds0 + (buf * BUF_HALFS + (2 + pl) * PLANE_HALFS + RPI * i * BK16) * 2);
                }
            }
            return;
        }
        u16* base = smem + buf * BUF_HALFS + RPI * IPW * uwave * BK16;
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const bool kv = k0 + ksrc[i] < p.K;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                const u16* pa = kv ? (const u16*)((const char*)(p.A + pl * p.a_plane + k0) + aoff[i]) : p.zero;
                const u16* pb = kv ? (const u16*)((const char*)(p.Bt + pl * p.b_plane + k0) + boff[i]) : p.zero;
                xv_dma16_ptr(pa, base + pl * PLANE_HALFS + RPI * i * BK16);
                xv_dma16_ptr(pb, base + (2 + pl) * PLANE_HALFS + RPI * i * BK16);
            }
        }
    };

    f32x16 acc[2][NB16];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB16; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int fsw = SWZ16(li);
    const int a_row = (wr * 64 + li) * BK16, b_row = (wc * 32 * NB16 + li) * BK16;
    if (nk > 0) gstage(0, 0);
    xv16_sync();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gstage(kt + 1, buf ^ 1);
        const u16* base = smem + buf * BUF_HALFS;
#pragma unroll
        for (int kb = 0; kb < BK16 / 16; ++kb) {
            const int pos = (((2 * kb + lh) ^ fsw) << 3);
            f32x4 af[2][2], bf[2][NB16];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
                af[pl][0] = *(const f32x4*)(base + pl * PLANE_HALFS + a_row + pos);
                af[pl][1] = *(const f32x4*)(base + pl * PLANE_HALFS + a_row + 32 * BK16 + pos);
#pragma unroll
                for (int nb = 0; nb < NB16; ++nb) bf[pl][nb] = *(const f32x4*)(base + (2 + pl) * PLANE_HALFS + b_row + nb * 32 * BK16 + pos);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < NB16; ++b) XV16_MFMA3_32X32X16(acc[a][b], af, bf, a, b);
        }
        xv16_sync();
    }

    const float out_scale = 1.0f / (xv_pow2_scale(p.a_amax ? *p.a_amax : 0u) * xv_pow2_scale(p.b_amax ? *p.b_amax : 0u));
    float bias_v[NB16];
#pragma unroll
    for (int b = 0; b < NB16; ++b) {
        int n = n0 + (wc * NB16 + b) * 32 + li;
        bias_v[b] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)      // scale + bias first, stores afterwards (why: the context-window kernel's epilogue, below)
#pragma unroll
        for (int b = 0; b < NB16; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = acc[a][b][r] * out_scale + bias_v[b];
    // (written out here and in the context-window kernel: a shared function changed the streams, profiles/gemm16_split_isa.txt)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB16; ++b) asm volatile("" : "+v"(acc[a][b]));      // keeps hipcc from sinking the pass back into the store blocks
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB16; ++b) {
            int n = n0 + (wc * NB16 + b) * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int m = m0 + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (m < p.M && n < p.N) p.C[(long)m * p.ldc + n] = acc[a][b][r];
            }
        }
    if (EPI == 1) xv_tile_stats_epilogue(acc, (float*)smem, tid, wr, wc, li, lh, m0, n0, p.M, p.N, tile_m, p.tiles_m, p.part);
    if (EPI == 2) xv_tile_bwd_stats_epilogue(acc, (float*)smem, tid, wr, wc, li, lh, m0, n0, p.M, p.N, tile_m, p.bwd);
}

// ---------------------------------------------------------------------------------------------
// Context-window ("conv") form of the NT kernel: K = taps x C with A row (m, tap j) = x row xrow(m) + j.
// The generic kernel re-reads every x row once per tap from L2 (its A image for tap j+1 is the image for tap j
// shifted by one row) - and the L2 request rate is what bounds it (PMC: 92 % L2 hits, TCP stalled on pending
// requests 45 % of the time, MFMA busy 40 %).  Here one LDS image of the x rows xrow(m0) .. xrow(m0+127)+taps-1
// for a 32-channel chunk serves all taps: the K loop runs channel chunk outer, tap inner, the MFMA A fragments
// of tap j are read at LDS row offset j, and only the weight tile (B) is staged per K-step.  The next chunk's
// x rows are fetched in `taps` slices, one per K-step, so every step issues about the same number of LDS-DMAs
// (5 per wave instead of 8 for taps = 5).  Rows of one tile may straddle segments: aoff(q) = xrow(m0+q) - xrow(m0)
// grows by (pitch - rps) at every crossing; the launcher falls back to the generic kernel when the rows of a
// tile do not fit the (BM + 32)-row image.
// LDS (128-row tile): A 2 x 2 planes x 160 rows x 64 B = 40 KB, B 2 x 2 planes x 128 x 64 B = 32 KB: two workgroups per CU.
// ---------------------------------------------------------------------------------------------
#define CONV_BPLANE (128 * 32)
#define CONV_BBUF (2 * CONV_BPLANE)

struct NT16ConvArgs {
    NT16Args g;                // tiles_m counts BM-row tiles (BM = 64 * WR)
    int taps, chunks;          // K = taps * C, chunks = C / 32
    long a_rows;               // rows of the A planes (reads beyond are zero)
};

// WR = row-waves per workgroup: 2 -> 128-row tile, 4 waves, 72 KB LDS, two workgroups per CU;
//                               4 -> 256-row tile, 8 waves, 104 KB LDS, one workgroup per CU: the weight tile staged per
//                                    K-step serves twice the rows (staging is the largest non-MFMA cost of this kernel).
template <int WR> struct ConvGeom {
    static constexpr int BM = 64 * WR;
    static constexpr int NW = 2 * WR;                 // waves
    static constexpr int AR = BM + 32;                // x rows per A image (tile + halo)
    static constexpr int APLANE = AR * 32;            // halfs per A plane image
    static constexpr int ABUF = 2 * APLANE;
    static constexpr int NG = AR / 16;                // 16-row DMA groups per plane
    static constexpr int BG = 8 / NW;                 // weight-tile DMA groups per wave
    static constexpr int LDS_HALFS = 2 * ABUF + 2 * CONV_BBUF;
};

// The context-window kernel contracts on v_mfma_f32_16x16x32_f16 (one instruction spans the whole 32-channel K-step; 4 x 4 accumulator
// blocks of 16 x 16 per wave), not v_mfma_f32_32x32x16_f16.  Operands: lane l reads row base + (l & 15), 16-byte chunk
// l >> 4 of a 64-byte row; chunk ^= 2 * ((row >> 2) & 1) puts the 16 lanes of every ds_read_b128 lane group on 16 distinct 4-bank columns
// for ANY base row (exhaustive check over the four lane groups and all 16 alignments; a context-window read shifts the rows by the tap) -
// the same involution is applied to the LDS-DMA source chunk.
// [measured] tdnn2 / tdnn3 at S1: forward 236 -> 218 us / 309 -> 300 us, data gradient 242 -> 234 us / 286 -> 270 us (+3 ... +8 %).
#define CONV_SWZ(row) ((((row) >> 2) & 1) << 1)

template <int EPI, int WR>
__global__ __launch_bounds__(128 * WR, 2) void xv_gemm16_nt_conv_kernel(NT16ConvArgs q) {
    typedef ConvGeom<WR> G;
    const NT16Args& p = q.g;
    extern __shared__ __attribute__((aligned(16))) u16 smem[];
    u16* const sA = smem;
    u16* const sB = smem + 2 * G::ABUF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int wr = wave >> 1, wc = wave & 1;
    const int t = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
    const int m0 = tile_m * G::BM, n0 = tile_n * 128;
    const int taps = q.taps, nc = q.chunks;
    const long C = p.lda;

    auto xrow = [&](int m) {
        int mm = min(m, p.M - 1);
        int seg = mm / p.a_rps, tt = mm - seg * p.a_rps;
        return (long)seg * p.a_pitch + tt;
    };
    const long xr0 = xrow(m0);
    // (nothing reads arow - the 32x32x16 form's LDS rows at tap 0 - but without it hipcc orders the scalar prologue of <EPI, 4> differently:
    // it stays until the kernel is next retimed, profiles/gemm16_split_isa.txt)
    int arow[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) arow[a] = (int)(xrow(m0 + wr * 64 + a * 32 + (lane & 31)) - xr0);

    // DMA lane geometry: one wave-instruction = 16 image rows x 64 B; lane -> row l>>2, 16-byte chunk l&3 (source chunk swizzled)
    const int drow = lane >> 2, dchunk = lane & 3;
    // B: rows 16*(BG*wave + i) + drow of the weight tile.  Byte offsets from the plane bases (xv_dma16: scalar base + 32-bit lane offset,
    // both planes share them); rows outside the operands read row 0 - their products are never stored or counted.
    unsigned boff[G::BG];
#pragma unroll
    for (int i = 0; i < G::BG; ++i) {
        const int row = 16 * (G::BG * wave + i) + drow;
        const int n = n0 + row;
        boff[i] = (unsigned)(((long)(n < p.N ? n : 0) * p.ldb + ((dchunk ^ CONV_SWZ(row)) << 3)) * 2);
    }
    const unsigned lds_b = xv_lds_addr(sB + 16 * G::BG * uwave * 32), lds_a = xv_lds_addr(sA);
    auto stage_b = [&](int cc, int j, int buf) {
        const long k0 = (long)j * C + cc * 32;
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) {
            const float* bbase = (const float*)(p.Bt + pl * p.b_plane + k0);
#pragma unroll
            for (int i = 0; i < G::BG; ++i) xv_dma16(bbase, boff[i], lds_b + (buf * CONV_BBUF + pl * CONV_BPLANE + 16 * i * 32) * 2);
        }
    };
    // A: NG row groups x 2 planes wave-instructions per chunk, id = plane*NG + group; slice `part` of `nparts`
    // hands ids part*NW + wave + s*NW*nparts to this wave.
    const int asrc = (dchunk ^ CONV_SWZ(drow)) << 3;      // (CONV_SWZ looks at bit 2 of the row: 16 * group does not touch it)
    auto stage_a = [&](int cc, int buf, int part, int nparts) {
        for (int id = part * G::NW + uwave; id < 2 * G::NG; id += G::NW * nparts) {
            const int pl = id >= G::NG ? 1 : 0, grp = id - G::NG * pl;
            const long xr = xr0 + 16 * grp + drow;
            const unsigned aoff = (unsigned)(((xr < q.a_rows ? xr : 0) * C + asrc) * 2);
            xv_dma16((const float*)(p.A + pl * p.a_plane + cc * 32), aoff, lds_a + (buf * G::ABUF + pl * G::APLANE + 16 * grp * 32) * 2);
        }
    };

    // (EPI: 0 or 1.  The BN-backward epilogue, EPI == 2, exists for the 32x32x16 accumulator layout only: nt16_form sends it to the generic kernel)
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lc = lane & 15, lg = lane >> 4;                 // fragment row / 8-channel chunk of this lane
    int arow16[4], b_off[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        arow16[qd] = (int)(xrow(m0 + wr * 64 + qd * 16 + lc) - xr0);
        const int rb = wc * 64 + qd * 16 + lc;
        b_off[qd] = rb * 32 + ((lg ^ CONV_SWZ(rb)) << 3);
    }
    stage_a(0, 0, 0, 1);
    stage_b(0, 0, 0);
    xv16_sync();
    int st = 0;
    for (int cc = 0; cc < nc; ++cc) {
        const u16* abase = sA + (cc & 1) * G::ABUF;
        for (int j = 0; j < taps; ++j, ++st) {
            if (j + 1 < taps) stage_b(cc, j + 1, (st + 1) & 1);
            else if (cc + 1 < nc) stage_b(cc + 1, 0, (st + 1) & 1);
            if (cc + 1 < nc) stage_a(cc + 1, (cc + 1) & 1, j, taps);
            const u16* bbase = sB + (st & 1) * CONV_BBUF;
            f32x4 af[2][4], bf[2][4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int ra = arow16[qd] + j;
                const int ao = ra * 32 + ((lg ^ CONV_SWZ(ra)) << 3);
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    af[pl][qd] = *(const f32x4*)(abase + pl * G::APLANE + ao);
                    bf[pl][qd] = *(const f32x4*)(bbase + pl * CONV_BPLANE + b_off[qd]);
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) XV16_MFMA3_16X16X32(acc[a][b], af, bf, a, b);
            xv16_sync();
        }
    }
    const float out_scale = 1.0f / (xv_pow2_scale(p.a_amax ? *p.a_amax : 0u) * xv_pow2_scale(p.b_amax ? *p.b_amax : 0u));
    // scale + bias in a pass of their own, THEN the stores: with both in one predicated block per element hipcc put the
    // s_waitcnt vmcnt(0) of the amax / bias loads in front of every store, and stores count on vmcnt - each store waited for
    // the previous one to retire
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int n = n0 + wc * 64 + b * 16 + lc;
        const float bias_v = (p.bias && n < p.N) ? p.bias[n] : 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[a][b][jj] = acc[a][b][jj] * out_scale + bias_v;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) asm volatile("" : "+v"(acc[a][b]));      // keeps hipcc from sinking the pass back into the store blocks
    // (the 16 x 16 block stores are written out here and in xv_gemm16_tn.hip: a shared function changed the streams, profiles/gemm16_split_isa.txt)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int n = n0 + wc * 64 + b * 16 + lc;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int m = m0 + wr * 64 + a * 16 + lg * 4 + jj;
                if (m < p.M && n < p.N) p.C[(long)m * p.ldc + n] = acc[a][b][jj];
            }
    }
    {
        const int half = wr >> 1;
        const int tiles128 = (p.M + 127) / 128;
        float* red = (float*)smem + half * 1024;
        if (EPI == 1)
            xv_tile_stats_epilogue16(acc, red, tid & 255, wr & 1, wc, lane, m0 + 128 * half, n0, p.M, p.N, (WR / 2) * tile_m + half, tiles128, p.part);
    }
}

// Does the context-window kernel apply?  K = taps*lda with whole 32-channel chunks, and the x rows of any BM-row tile
// (one extra (pitch - rps) per segment crossing, plus the taps) fit the A image of BM + 32 rows.
static bool conv_form_applies(const XvGemm16NT& g, int bm, int* taps_out) {
    if (g.lda % 32 != 0 || g.K % g.lda != 0) return false;
    const int taps = (int)(g.K / g.lda);
    if (taps < 2 || g.a_pitch < g.a_rps) return false;
    const long crossings = (bm - 1) / g.a_rps + 1;
    const long span = (bm - 1) + (long)(g.a_pitch - g.a_rps) * crossings + (taps - 1);
    if (span >= bm + 32) return false;
    *taps_out = taps;
    return true;
}

// The launch form of an NT problem, stated once: xv_launch_gemm16_nt runs it, xv_debug_gemm16_nt_form reports it.
struct NT16Form {
    int conv;                  // 1: the context-window kernel, 0: the generic one
    int bm;                    // rows of a tile (128; 256 for the context-window kernel with 4 row-waves)
    int taps, chunks;          // context-window kernel: K = taps * lda, chunks = lda / 32 (0, 0 for the generic kernel)
    int tiles_m, tiles_n;
    int nk;                    // K-steps of 32 halfs (context-window kernel: taps * chunks)
    int last_valid;            // halfs of the last K-step that lie inside K rounded up to 8 (8 ... 32)
};

// what both the launcher and the hook refuse about the shape of a problem (pointers are the launcher's own business)
static int nt16_check_shape(const XvGemm16NT& g) {
    XV_REQUIRE(g.lda % 8 == 0 && g.ldb % 8 == 0, "gemm16_nt: lda/ldb must be multiples of 8 (lda=%ld ldb=%ld)", g.lda, g.ldb);
    XV_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0 && g.a_rps > 0, "gemm16_nt: empty problem");
    // xv_dma16 addresses every row of a plane as a 32-bit byte offset from the plane's base
    XV_REQUIRE(((long)xv_cdiv(g.M, g.a_rps) * g.a_pitch + 1) * g.lda * 2 < (1L << 32) && ((long)g.N + 1) * g.ldb * 2 < (1L << 32),
               "gemm16_nt: a plane spans 4 GB or more (M=%d a_pitch=%d lda=%ld N=%d ldb=%ld): split the batch", g.M, g.a_pitch, g.lda, g.N, g.ldb);
    return 0;
}

// conv_wr: XvEnv::conv_wr (XV_CONV_WR=4 (experiments, tests) forces 256-row tiles wherever they apply).  bwd: the BN-backward epilogue
// (an off-by-default experiment) is written for the 32x32x16 accumulator layout, which the context-window kernel (16x16x32) does not
// have: such a launch takes the generic kernel.
// [measured] 256-row tiles (XV_CONV_WR=4) are 5-7 % slower at S1 (tdnn2/3 forward 270 vs 291 TF): 384 one-per-CU
// workgroups on 256 CUs leave half the chip idle for the second round, which costs more than the halved weight-tile
// staging saves.  128-row tiles stay the default.
static NT16Form nt16_form(const XvGemm16NT& g, bool bwd, int conv_wr) {
    NT16Form f;
    const int Kp = (int)xv_align(g.K, 8);
    int taps = 0;
    f.conv = 1;
    if (!bwd && conv_wr == 4 && conv_form_applies(g, 256, &taps)) f.bm = 256;
    else if (!bwd && conv_form_applies(g, 128, &taps)) f.bm = 128;
    else { f.conv = 0; f.bm = 128; taps = 0; }
    f.taps = taps;
    f.chunks = f.conv ? (int)(g.lda / 32) : 0;
    f.tiles_m = xv_cdiv(g.M, f.bm);
    f.tiles_n = xv_cdiv(g.N, 128);
    f.nk = f.conv ? f.taps * f.chunks : xv_cdiv(Kp, BK16);
    f.last_valid = f.conv ? 32 : Kp - (f.nk - 1) * BK16;
    return f;
}

extern "C" int xv_debug_gemm16_nt_form(int M, int N, int K, int lda, int a_rps, int a_pitch, int stats, int bwd, int conv_wr, int out[8]) {
    XV_REQUIRE(out, "xv_debug_gemm16_nt_form: out is NULL");
    XV_REQUIRE(conv_wr == 0 || conv_wr == 2 || conv_wr == 4, "xv_debug_gemm16_nt_form: conv_wr must be 0, 2 or 4");
    XV_REQUIRE(!(stats && bwd), "gemm16_nt: one epilogue at a time");
    XvGemm16NT g = {};
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = K; g.a_rps = a_rps; g.a_pitch = a_pitch;      // (ldb = K: the op-level wrappers' weight planes)
    if (int rc = nt16_check_shape(g)) return rc;
    const NT16Form f = nt16_form(g, bwd != 0, conv_wr == 4 ? 4 : 0);
    out[0] = f.conv; out[1] = f.bm; out[2] = f.taps; out[3] = f.chunks; out[4] = f.tiles_m; out[5] = f.tiles_n; out[6] = f.nk; out[7] = f.last_valid;
    return 0;
}

// Launches the instantiation of a kernel family that a problem's epilogue asks for: kern[EPI], EPI = 1 with forward BN statistics,
// 2 with BN-backward reductions, else 0.
template <class Args, size_t NEPI>
static int launch_epi(void (*const (&kern)[NEPI])(Args), const XvGemm16NT& g, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args& args) {
    const size_t epi = g.bn_part ? 1 : g.bwd_part ? 2 : 0;
    XV_REQUIRE(epi < NEPI, "gemm16_nt: the kernel picked has no epilogue %d", (int)epi);
    hipLaunchKernelGGL(kern[epi], grid, block, lds, s, args);
    XV_LAUNCH_CHECK();
    return 0;
}

template <int WR>
static int launch_conv(hipStream_t s, const XvGemm16NT& g, const NT16Args& p, const NT16Form& f) {
    // (no <2, WR>: nt16_form never picks this kernel for a BN-backward launch)
    static void (*const kern[])(NT16ConvArgs) = {xv_gemm16_nt_conv_kernel<0, WR>, xv_gemm16_nt_conv_kernel<1, WR>};
    NT16ConvArgs q;
    q.g = p; q.taps = f.taps; q.chunks = f.chunks;      // (p.tiles_m counts the form's BM-row tiles)
    q.a_rows = (long)xv_cdiv(g.M, g.a_rps) * g.a_pitch;
    const size_t lds = (size_t)ConvGeom<WR>::LDS_HALFS * sizeof(u16);
    static bool attr_done = false;
    if (!attr_done) {
        for (auto k : kern) XV_CHECK_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done = true;
    }
    return launch_epi(kern, g, dim3(f.tiles_m * f.tiles_n), dim3(128 * WR), lds, s, q);
}

int xv_launch_gemm16_nt(hipStream_t s, const XvGemm16NT& g) {
    static void (*const kern[])(NT16Args) = {xv_gemm16_nt_kernel<0>, xv_gemm16_nt_kernel<1>, xv_gemm16_nt_kernel<2>};
    if (int rc = nt16_check_shape(g)) return rc;
    XV_REQUIRE(((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.Bt % 16) == 0 && g.a_plane % 8 == 0 && g.b_plane % 8 == 0,
               "gemm16_nt: planes must be 16-byte aligned");
    const bool bwd = g.bwd_part != nullptr;
    XV_REQUIRE(!(bwd && g.bn_part), "gemm16_nt: one epilogue at a time");
    XV_REQUIRE(!bwd || (g.bwd_z && g.bwd_scale && g.bwd_shift && g.bwd_mean && g.bwd_invstd),
               "gemm16_nt: incomplete BN-backward epilogue arguments");
    const XvEnv* env = xv_env();
    if (!env) return 2;
    const NT16Form f = nt16_form(g, bwd, env->conv_wr);
    NT16Args p;
    p.A = (const u16*)g.A; p.lda = g.lda; p.a_plane = g.a_plane; p.a_rps = g.a_rps; p.a_pitch = g.a_pitch;
    p.Bt = (const u16*)g.Bt; p.ldb = g.ldb; p.b_plane = g.b_plane;
    p.C = g.C; p.ldc = g.ldc; p.M = g.M; p.N = g.N; p.K = (int)xv_align(g.K, 8);
    p.tiles_m = f.tiles_m; p.tiles_n = f.tiles_n;
    p.bias = g.bias; p.part = g.bn_part; p.a_amax = g.a_amax; p.b_amax = g.b_amax;
    p.zero = (const u16*)xv_zero_page();
    if (!p.zero) return 1;
    p.bwd = XvBwdStats{g.bwd_z, g.bwd_scale, g.bwd_shift, g.bwd_mean, g.bwd_invstd, g.bwd_part};
    XvProfScope prof(s, g.bn_part ? 3 : 4, 2.0 * g.M * g.N * g.K);
    if (f.conv) return f.bm == 256 ? launch_conv<4>(s, g, p, f) : launch_conv<2>(s, g, p, f);
    return launch_epi(kern, g, dim3(p.tiles_m * p.tiles_n), dim3(256), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// Public op-level wrappers (include/xvector_hip.h, "split precision")
// ---------------------------------------------------------------------------------------------
extern "C" int xv_affine_forward_f16x3(void* stream, const void* x_planes, size_t x_plane_stride, const uint32_t* x_amax, int segs, int t_in,
                                       int c_ld, int k, const void* wt_planes, size_t wt_plane_stride, const uint32_t* wt_amax,
                                       const float* bias, float* z, int o, int ldz, float* bn_part) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_in >= k && c_ld > 0 && o > 0 && ldz >= o, "affine_forward_f16x3: bad shape (t_in=%d k=%d)", t_in, k);
    XvGemm16NT g = {};
    g.A = x_planes; g.lda = c_ld; g.a_plane = (long)x_plane_stride; g.a_rps = t_in - k + 1; g.a_pitch = t_in;
    g.Bt = wt_planes; g.ldb = (long)k * c_ld; g.b_plane = (long)wt_plane_stride;
    g.C = z; g.ldc = ldz; g.M = segs * (t_in - k + 1); g.N = o; g.K = k * c_ld;
    g.bias = bias; g.bn_part = bn_part; g.a_amax = x_amax; g.b_amax = wt_amax;
    return xv_launch_gemm16_nt((hipStream_t)stream, g);
}

// The data gradient as an NT problem: dx [segs*(t_out+k-1)][c] = padded dz planes (k-1 zero rows on either side of a segment) x flipped weights.
// bwd: null, or the BN-backward epilogue's arguments (all of them).
static int dgrad16(const char* who, void* stream, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax, int segs, int t_out, int o_ld,
                   int k, const void* wf_planes, size_t wf_plane_stride, const uint32_t* wf_amax, float* dx, int c, const XvBwdStats* bwd) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_out >= 1 && o_ld > 0 && c > 0, "%s: bad shape", who);
    XV_REQUIRE(!bwd || (bwd->z && bwd->scale && bwd->shift && bwd->mean && bwd->invstd && bwd->part), "%s: null BN argument", who);
    XvGemm16NT g = {};
    g.A = dz_planes; g.lda = o_ld; g.a_plane = (long)dz_plane_stride; g.a_rps = t_out + k - 1; g.a_pitch = t_out + 2 * (k - 1);
    g.Bt = wf_planes; g.ldb = (long)k * o_ld; g.b_plane = (long)wf_plane_stride;
    g.C = dx; g.ldc = c; g.M = segs * (t_out + k - 1); g.N = c; g.K = k * o_ld;
    g.a_amax = dz_amax; g.b_amax = wf_amax;
    if (bwd) { g.bwd_z = bwd->z; g.bwd_scale = bwd->scale; g.bwd_shift = bwd->shift; g.bwd_mean = bwd->mean; g.bwd_invstd = bwd->invstd; g.bwd_part = bwd->part; }
    return xv_launch_gemm16_nt((hipStream_t)stream, g);
}

extern "C" int xv_affine_dgrad_f16x3(void* stream, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax, int segs, int t_out,
                                     int o_ld, int k, const void* wf_planes, size_t wf_plane_stride, const uint32_t* wf_amax, float* dx,
                                     int c) {
    return dgrad16("affine_dgrad_f16x3", stream, dz_planes, dz_plane_stride, dz_amax, segs, t_out, o_ld, k, wf_planes, wf_plane_stride, wf_amax, dx,
                   c, nullptr);
}

// xv_affine_dgrad_f16x3 whose epilogue also produces the per-tile partials of the BN backward of the layer that owns dx
// (dx = d a of a BN+ReLU layer with pre-BN output z_below [rows][c]): part [ceil(rows/128)][3][c] = sum dd | sum dd*xhat | max |dd|.
extern "C" int xv_affine_dgrad_bnstats_f16x3(void* stream, const void* dz_planes, size_t dz_plane_stride, const uint32_t* dz_amax, int segs,
                                             int t_out, int o_ld, int k, const void* wf_planes, size_t wf_plane_stride,
                                             const uint32_t* wf_amax, float* dx, int c, const float* z_below, const float* scale,
                                             const float* shift, const float* mean, const float* invstd, float* part) {
    const XvBwdStats bwd = {z_below, scale, shift, mean, invstd, part};
    return dgrad16("affine_dgrad_bnstats_f16x3", stream, dz_planes, dz_plane_stride, dz_amax, segs, t_out, o_ld, k, wf_planes, wf_plane_stride,
                   wf_amax, dx, c, &bwd);
}
