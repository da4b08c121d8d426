// fp32 MFMA GEMM, "TN" shape, for the TDNN hot path (gfx950 / CDNA4 only):
//
//  TN  P[m][n] = sum_r A[amap(r)][m] * B[bmap(r)][n]
//      weight gradients (reduction over the ~25k (chunk,frame) rows), split over r.
//
// (The NT shape - forward, data gradients, logits - is xv_gemm_nt.hip; the spliced row map and the MFMA operand maps are described there.)
// Here: the 128 x 128-tile kernel, the 160-row kernel of tdnn1's weight gradient, their planner and launcher, the slab sum behind them, and
// the xv_affine_wgrad entry points.
//
// Tile and workgroup as in the NT kernels: 128x128 output tile, 256 threads = 4 waves (2x2), each wave a 64x64 sub-tile as 2x2
// v_mfma_f32_32x32x2_f32 accumulators, K-step XV_TILE_K = 16 reduction rows, operand tiles staged by LDS-DMA (xv_dma16, xv_handoff.h) into a
// double-buffered 32 KB LDS image [r][128] (below), XV_WGS_PER_CU = 4 workgroups per CU (xv_gemm.h).
#include "xv_common.h"
#include <type_traits>
#include "xv_gemm.h"
#include "xv_gemm_tile.h"
#include <algorithm>

#define BM XV_TILE_M
#define BN XV_TILE_N
#define BK XV_TILE_K
#define TN_RPT (BK / 8)              // reduction rows staged per thread (2 or 4)

// -------------------------------------------------------------------------------------
// TN: weight gradients
// -------------------------------------------------------------------------------------
struct TNArgs {
    const float* A; long lda; int a_pitch;
    const float* B; long ldb; int b_pitch;
    int rps; float inv_rps;
    float* P;
    int M, N, R, r_chunk;
    int tiles_m, tiles_n;
    const float* zero;
    int ahead;      // K-step schedule (see the kernel)
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// LDS image [r][128] (output index contiguous, exactly as it sits in HBM: no transpose).
// Fragment reads are ds_read_b64: lane i of a lane-half takes output rows 2i and 2i+1 of the
// wave's 64 at reduction row r = 2*ks + half, which feed the two 32x32 accumulators in that
// direction (the MFMA only needs A and B to agree on r).  So accumulator (a,b) register reg of
// lane l holds  m = m0 + wr*64 + 2*row(reg,l) + a,  n = n0 + wc*64 + 2*(l&31) + b.
// (Round 5 built wave groups on top of this kernel - 512 / 1 024-thread workgroups whose groups take consecutive reduction chunks of ONE tile
// and add their accumulators through LDS before a single slab store, 1/2 or 1/4 of the slab bytes: parity-green, no faster alone, 3 % slower
// in the step; removed.  profiles/r05_tn_wave_groups.txt, DESIGN.md Appendix A.)
#define XV_TN_STAGES 2
#ifndef XV_TN_AHEAD_MIN
#define XV_TN_AHEAD_MIN 16      // K-steps per workgroup from which the two-steps-ahead DMA schedule is used (xv_launch_gemm_tn; 96 until the staging addresses went scalar)
#endif
__global__ __launch_bounds__(256, XV_WGS_PER_CU) void xv_gemm_tn_kernel(TNArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[XV_TN_STAGES * 2 * BK * BM];   // [slot][A|B][BK][128]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    // 1-D grid over (split, tile): after the XCD swizzle every XCD owns a contiguous run, i.e. whole
    // reduction chunks, so the rows of A and B that one chunk touches are fetched into ONE L2
    // (the (tiles, splits) grid of the first build spread every chunk over all 8 XCDs: 51 % hits).
    const int v = xcd_swizzle(blockIdx.x, gridDim.x);
    const int tiles = p.tiles_m * p.tiles_n;
    const int split = v / tiles, t = v - split * tiles;
    const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int r_begin = split * p.r_chunk;
    const int r_end = min(p.R, r_begin + p.r_chunk);
    const int nk = (r_end - r_begin + BK - 1) / BK;

    // LDS-DMA staging: one wave-instruction = 1 KiB = two whole [r][128] rows of the image; lane l lands on
    // row 2*(RPT*wave+i) + l/32, columns 4*(l%32)..+3.  The reduction-row -> address map (spliced view)
    // is evaluated per lane without an integer divide (r < 2^24, float quotient off by <= 1).
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int lc = (lane & 31) * 4;
    const bool a_cv = (m0 + lc) < p.M, b_cv = (n0 + lc) < p.N;
    const float* __restrict__ zp = p.zero;
    const float* abase = p.A + (a_cv ? m0 + lc : 0);
    const float* bbase = p.B + (b_cv ? n0 + lc : 0);
    auto gstage_ragged = [&](int kt, int buf) {      // a K-step with rows at or beyond r_end: those read the zero page (they are summed)
        float* sa = smem + buf * (2 * BK * BM) + 2 * TN_RPT * uwave * BM;
        float* sb = sa + BK * BM;
#pragma unroll
        for (int i = 0; i < TN_RPT; ++i) {
            int r = r_begin + kt * BK + 2 * (TN_RPT * wave + i) + (lane >> 5);
            bool rv = r < r_end;
            int seg = (int)((float)r * p.inv_rps);
            int tt = r - seg * p.rps;
            seg += (tt >= p.rps) - (tt < 0);
            tt = r - seg * p.rps;
            const float* pa = (rv && a_cv) ? abase + ((long)seg * p.a_pitch + tt) * p.lda : zp;
            const float* pb = (rv && b_cv) ? bbase + ((long)seg * p.b_pitch + tt) * p.ldb : zp;
            xv_dma16_ptr(pa, sa + 2 * i * BM);
            xv_dma16_ptr(pb, sb + 2 * i * BN);
        }
    };
    // Full K-steps (every row below r_end): the K-step's first row r0 is resolved to (segment, frame) in SCALAR registers and advanced
    // there - frame += BK, and on crossing the segment's last frame the base also skips the rows between two segments; a lane adds its
    // constant offset (its row j of the 16, its four columns), taken from the "next segment" copy when frame + j lies beyond the segment:
    // one compare and two selects per DMA pair.  (The first build resolved row -> (segment, frame) -> 64-bit address from scratch for every
    // K-step: ~40 vector instructions per wave and step; rounds 1-4 advanced per-lane offsets: 14 - and a vector instruction takes its ALU
    // cycles from the fp32 MFMAs.)  Columns outside the matrix read column 0: their products are never stored.
    const bool steady = p.rps >= BK;      // at most one segment boundary per step
    int jrow[TN_RPT];
    unsigned aoff[TN_RPT], boff[TN_RPT], aoff_w[TN_RPT], boff_w[TN_RPT];
    const unsigned a_step = (unsigned)(BK * p.lda * 4), b_step = (unsigned)(BK * p.ldb * 4);
    const unsigned a_skip = (unsigned)((long)(p.a_pitch - p.rps) * p.lda * 4), b_skip = (unsigned)((long)(p.b_pitch - p.rps) * p.ldb * 4);
#pragma unroll
    for (int i = 0; i < TN_RPT; ++i) {
        jrow[i] = 2 * (TN_RPT * wave + i) + (lane >> 5);
        aoff[i] = (unsigned)(((long)jrow[i] * p.lda + (a_cv ? m0 + lc : 0)) * 4);
        boff[i] = (unsigned)(((long)jrow[i] * p.ldb + (b_cv ? n0 + lc : 0)) * 4);
        aoff_w[i] = aoff[i] + a_skip;
        boff_w[i] = boff[i] + b_skip;
    }
    // scalar state of the next K-step to stage: frame of its first row within its segment, byte offsets of that row in A and B
    int s_tt;
    unsigned s_a, s_b;
    {
        const int r0 = __builtin_amdgcn_readfirstlane(min(r_begin, p.R - 1));
        const int seg0 = r0 / p.rps;
        s_tt = r0 - seg0 * p.rps;
        s_a = (unsigned)(((long)seg0 * p.a_pitch + s_tt) * p.lda * 4);
        s_b = (unsigned)(((long)seg0 * p.b_pitch + s_tt) * p.ldb * 4);
    }
    const unsigned lds0 = xv_lds_addr(smem + 2 * TN_RPT * uwave * BM);
    auto gstage = [&](int kt, int buf) {
        if (!steady || r_begin + (kt + 1) * BK > r_end) {
            gstage_ragged(kt, buf);
            return;
        }
        // (kt counts up by one per call, so the scalar state is at step kt here)
        const float* sa = (const float*)((const char*)p.A + s_a);
        const float* sb = (const float*)((const char*)p.B + s_b);
        const int thr = p.rps - s_tt;      // rows j >= thr of this K-step belong to the next segment
#pragma unroll
        for (int i = 0; i < TN_RPT; ++i) {
            const bool w = jrow[i] >= thr;
            xv_dma16(sa, w ? aoff_w[i] : aoff[i], lds0 + (buf * (2 * BK * BM) + 2 * i * BM) * 4);
            xv_dma16(sb, w ? boff_w[i] : boff[i], lds0 + (buf * (2 * BK * BM) + BK * BM + 2 * i * BN) * 4);
        }
        s_tt += BK;
        s_a += a_step;
        s_b += b_step;
        if (s_tt >= p.rps) { s_tt -= p.rps; s_a += a_skip; s_b += b_skip; }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int a_off = lh * BM + wr * 64 + 2 * li;
    const int b_off = lh * BN + wc * 64 + 2 * li;
    // Schedule of a K-step, two forms.  AHEAD: all sixteen fragment reads of stage kt, the first sixteen MFMAs, then - in mid-step - the
    // wait for the DMA of stage kt + 1, the workgroup barrier (every wave has read stage kt: its slot is free; stage kt + 1 is visible),
    // the DMA of stage kt + 2 into the slot just freed, and the other sixteen MFMAs: a stage's loads have a whole K-step to land.
    // sched_barrier pins the order.  Plain: the DMA of stage kt + 1 at the top of step kt, wait + barrier where hipcc puts them (right
    // behind the fragment reads - the last MEMORY operations of the step - i.e. in front of all 32 MFMAs).  The launcher chooses per
    // problem (TNArgs::ahead).
    if (nk > 0) gstage(0, 0);
    xv_dma_wait_all();      // (the compiler does not see xv_dma16's loads)
    __syncthreads();
    auto k_loop = [&](auto ahead_c) {
        constexpr bool AHEAD = decltype(ahead_c)::value;
        if (AHEAD && nk > 1) gstage(1, 1);
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (!AHEAD && kt + 1 < nk) gstage(kt + 1, buf ^ 1);
            const float* sa = smem + buf * (2 * BK * BM) + a_off;
            const float* sb = smem + buf * (2 * BK * BM) + BK * BM + b_off;
            f32x2 af[BK / 4], bf[BK / 4], an[BK / 4], bn[BK / 4];
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                af[j] = *(const f32x2*)(sa + 2 * j * BM);
                bf[j] = *(const f32x2*)(sb + 2 * j * BN);
            }
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                an[j] = *(const f32x2*)(sa + 2 * (BK / 4 + j) * BM);
                bn[j] = *(const f32x2*)(sb + 2 * (BK / 4 + j) * BN);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].x, bf[j].x, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].x, bf[j].y, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].y, bf[j].x, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j].y, bf[j].y, acc[1][1], 0, 0, 0);
            }
            if (AHEAD) {
                __builtin_amdgcn_sched_barrier(0);
                xv_dma_wait_all();
                __syncthreads();
                if (kt + 2 < nk) gstage(kt + 2, buf);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(an[j].x, bn[j].x, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(an[j].x, bn[j].y, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(an[j].y, bn[j].x, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(an[j].y, bn[j].y, acc[1][1], 0, 0, 0);
            }
            if (!AHEAD) {
                xv_dma_wait_all();
                __syncthreads();
            }
        }
    };
    if (p.ahead) k_loop(std::true_type{});
    else k_loop(std::false_type{});

    // (Summing the split partials of DIFFERENT workgroups inside this kernel - the last arrival adds the others' slabs - was built and dropped in
    // round 3: one workgroup reads splits x 64 KB serially at the end of the launch; DESIGN.md Appendix A.)
    // The slab tile goes out through the group's (idle) staging LDS in whole rows of 16 bytes per lane, as in nt_store_tile_rows: pass a writes
    // the tile's rows 2 q + a (q = wr * 32 + the accumulator's row) as a [64][128] image - a lane holds two neighbouring columns of a row, one
    // ds_write_b64 - and every thread stores eight float4 of whole rows (16 store instructions per lane instead of 32 eight-byte ones).
    // (M and N are multiples of 4 and the slab base is 16-byte aligned: xv_launch_gemm_tn.)
    float* P = p.P + (long)split * p.M * p.N;
    __syncthreads();                              // (every fragment read of the last stage is done)
    float* wbase = smem + (wr * 32 + 4 * lh) * BN + wc * 64 + 2 * li;
    const int rq = tid >> 5, cq = (tid & 31) * 4;
    const bool col_ok = n0 + cq < p.N;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x2 v = {acc[a][0][r], acc[a][1][r]};
            *(f32x2*)(wbase + ((r & 3) + 8 * (r >> 2)) * BN) = v;
        }
        __syncthreads();
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *(const f32x4*)(smem + (rq + 8 * i) * BN + cq);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int m = m0 + 2 * (rq + 8 * i) + a;
            if (m < p.M && col_ok) *(f32x4*)(P + (long)m * p.N + n0 + cq) = v[i];
        }
        if (a == 0) __syncthreads();
    }
}


// ---- weight gradient of a layer with 129 ... 160 input rows (tdnn1: 5 taps x 32 padded feature channels) ----------------------------
// On 128 x 128 tiles those rows are two tiles of which 3/8 of the second is real: 1.6 x the MFMAs, on the last weight gradient of every step.
// Here a workgroup owns ALL rows x 128 columns: wave w = columns 32 w .. 32 w + 31, five 32 x 32 accumulators down the rows (rows 0..127
// interleaved in pairs as in xv_gemm_tn_kernel - one ds_read_b64 feeds two of them - rows 128..159 straight).  LDS image per stage: A [16][160]
// (linear: an LDS-DMA piece of 1 KB is 1.6 rows, every lane resolves its own (row, column)) + B [16][128]; 2 workgroups per CU, 512 of them =
// one round.  (67 -> 55 us alone at S1; workgroup counts and schedules tried: DESIGN.md Appendix B, note 8.)
#define TNW_M 160
#define TNW_A_PIECES (BK * TNW_M / 256)      // 1 KB pieces per stage: 10
#define TNW_B_PIECES (BK * BN / 256)         // 8
#define TNW_WGS 512                         // (768 / 1 024 workgroups were slower alone: Appendix B, note 8; 256 / 384 no different in the step: round 6)
__global__ __launch_bounds__(256, 2) void xv_gemm_tn160_kernel(TNArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[2 * BK * (TNW_M + BN)];      // [slot][A [16][160] | B [16][128]]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int v = xcd_swizzle(blockIdx.x, gridDim.x);
    const int split = v / p.tiles_n, tile_n = v - split * p.tiles_n;
    const int n0 = tile_n * BN;
    const int r_begin = split * p.r_chunk;
    const int r_end = min(p.R, r_begin + p.r_chunk);
    const int nk = (r_end - r_begin + BK - 1) / BK;
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const float* __restrict__ zp = p.zero;
    constexpr int SLOT = BK * (TNW_M + BN);
    // pieces: A piece q (q = wave, wave + 4, wave + 8 < 10) = floats [256 q, 256 q + 256) of the stage's A image; B piece q (q = 2 wave, 2 wave + 1) =
    // rows 2 q, 2 q + 1 of B.  Per lane and piece: the reduction row within the K-step and the byte offset of its 16 bytes in that row.
    constexpr int NA = 3, NB = 2;
    int rowA[NA], rowB[NB];
    unsigned colA[NA], colB[NB];
    bool pieceA[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int q = wave + 4 * i;
        pieceA[i] = q < TNW_A_PIECES;
        const int f = 256 * q + 4 * lane;
        rowA[i] = f / TNW_M;
        const int c = f - rowA[i] * TNW_M;
        colA[i] = (unsigned)((c < p.M ? c : 0) * 4);      // columns beyond M (M < 160) read column 0: their products are never stored
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        rowB[i] = 2 * (NB * wave + i) + (lane >> 5);
        const int c = n0 + 4 * (lane & 31);
        colB[i] = (unsigned)((c < p.N ? c : 0) * 4);
    }
    // a K-step with rows at or beyond r_end (they read the zero page: they are summed) or of a layer with segments shorter than a K-step: every
    // lane resolves reduction row -> (segment, frame) -> address
    auto gstage_ragged = [&](int kt, int buf) {
        float* sa = smem + buf * SLOT;
        float* sb = sa + BK * TNW_M;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (!pieceA[i]) continue;      // (uniform per wave)
            const int r = r_begin + kt * BK + rowA[i];
            int seg = (int)((float)r * p.inv_rps);
            int tt = r - seg * p.rps;
            seg += (tt >= p.rps) - (tt < 0);
            tt = r - seg * p.rps;
            const float* pa = r < r_end ? (const float*)((const char*)(p.A + ((long)seg * p.a_pitch + tt) * p.lda) + colA[i]) : zp;
            xv_dma16_ptr(pa, sa + 256 * (uwave + 4 * i));
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int r = r_begin + kt * BK + rowB[i];
            int seg = (int)((float)r * p.inv_rps);
            int tt = r - seg * p.rps;
            seg += (tt >= p.rps) - (tt < 0);
            tt = r - seg * p.rps;
            const float* pb = r < r_end ? (const float*)((const char*)(p.B + ((long)seg * p.b_pitch + tt) * p.ldb) + colB[i]) : zp;
            xv_dma16_ptr(pb, sb + 256 * (NB * uwave + i));
        }
    };
    // full K-steps: the scheme of xv_gemm_tn_kernel - the K-step's first row lives in scalar registers as (frame within its segment, byte
    // offsets in A and B) and advances there; a lane adds the constant offset of its row of the 16 and of its columns, from the "next
    // segment" copy when frame + row lies beyond the segment.  (Rounds 4's form resolved every lane's row with a float multiply, two
    // conversions and 64-bit address arithmetic per piece: ~100 vector instructions per wave and K-step beside 20 MFMAs.)
    const bool steady = p.rps >= BK;
    const unsigned a_skip = (unsigned)((long)(p.a_pitch - p.rps) * p.lda * 4), b_skip = (unsigned)((long)(p.b_pitch - p.rps) * p.ldb * 4);
    const unsigned a_step = (unsigned)(BK * p.lda * 4), b_step = (unsigned)(BK * p.ldb * 4);
    unsigned offA[NA], offA_w[NA], offB[NB], offB_w[NB];
#pragma unroll
    for (int i = 0; i < NA; ++i) { offA[i] = (unsigned)((long)rowA[i] * p.lda * 4) + colA[i]; offA_w[i] = offA[i] + a_skip; }
#pragma unroll
    for (int i = 0; i < NB; ++i) { offB[i] = (unsigned)((long)rowB[i] * p.ldb * 4) + colB[i]; offB_w[i] = offB[i] + b_skip; }
    int s_tt;
    unsigned s_a, s_b;
    {
        const int r0 = __builtin_amdgcn_readfirstlane(min(r_begin, p.R - 1));
        const int seg0 = r0 / p.rps;
        s_tt = r0 - seg0 * p.rps;
        s_a = (unsigned)(((long)seg0 * p.a_pitch + s_tt) * p.lda * 4);
        s_b = (unsigned)(((long)seg0 * p.b_pitch + s_tt) * p.ldb * 4);
    }
    const unsigned lds_a0 = xv_lds_addr(smem + 256 * uwave), lds_b0 = xv_lds_addr(smem + BK * TNW_M + 256 * NB * uwave);
    auto gstage = [&](int kt, int buf) {
        if (!steady || r_begin + (kt + 1) * BK > r_end) {
            gstage_ragged(kt, buf);
            return;
        }
        // (kt counts up by one per call, so the scalar state is at step kt here)
        const float* sa = (const float*)((const char*)p.A + s_a);
        const float* sb = (const float*)((const char*)p.B + s_b);
        const int thr = p.rps - s_tt;      // rows >= thr of this K-step belong to the next segment
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (!pieceA[i]) continue;      // (uniform per wave)
            xv_dma16(sa, rowA[i] >= thr ? offA_w[i] : offA[i], lds_a0 + (buf * SLOT + 256 * 4 * i) * 4);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) xv_dma16(sb, rowB[i] >= thr ? offB_w[i] : offB[i], lds_b0 + (buf * SLOT + 256 * i) * 4);
        s_tt += BK;
        s_a += a_step;
        s_b += b_step;
        if (s_tt >= p.rps) { s_tt -= p.rps; s_a += a_skip; s_b += b_skip; }
    };

    f32x16 acc[5];
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;
    const int a_off = lh * TNW_M + 2 * li;              // rows 2 li, 2 li + 1 (and + 64) of reduction row 2 ks + lh
    const int a4_off = lh * TNW_M + 128 + li;           // row 128 + li
    const int b_off = lh * BN + 32 * wave + li;
    // (plain double buffering: the two-steps-ahead form of xv_gemm_tn_kernel was slower here, Appendix B note 8)
    if (nk > 0) gstage(0, 0);
    xv_dma_wait_all();
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gstage(kt + 1, buf ^ 1);
        const float* sa = smem + buf * SLOT;
        const float* sb = sa + BK * TNW_M;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x2 a01[BK / 4], a23[BK / 4];
            float a4[BK / 4], bf[BK / 4];
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                const int ks = h * (BK / 4) + j;
                a01[j] = *(const f32x2*)(sa + 2 * ks * TNW_M + a_off);
                a23[j] = *(const f32x2*)(sa + 2 * ks * TNW_M + a_off + 64);
                a4[j] = sa[2 * ks * TNW_M + a4_off];
                bf[j] = sb[2 * ks * BN + b_off];
            }
#pragma unroll
            for (int j = 0; j < BK / 4; ++j) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01[j].x, bf[j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a01[j].y, bf[j], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a23[j].x, bf[j], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a23[j].y, bf[j], acc[3], 0, 0, 0);
                acc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[j], bf[j], acc[4], 0, 0, 0);
            }
        }
        xv_dma_wait_all();
        __syncthreads();
    }
    // slab [split][M][N]: accumulator a < 4, register r of lane (li, lh) = row 64 (a / 2) + 2 row(r, lh) + a % 2; accumulator 4 = row 128 + row(r, lh);
    // column n0 + 32 wave + li
    float* P = p.P + (long)split * p.M * p.N;
    const int n = n0 + 32 * wave + li;
    if (n < p.N) {
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ri = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int m = a < 4 ? 64 * (a >> 1) + 2 * ri + (a & 1) : 128 + ri;
                if (m < p.M) P[(long)m * p.N + n] = acc[a][r];
            }
    }
}

static bool tn_wide_rows(int M) { return M > BM && M <= TNW_M; }

// Decomposition of a weight-gradient GEMM: `splits` slabs (workgroups per tile), `chunk` reduction rows per workgroup.  One co-resident round:
// XV_WGS_PER_CU (4) workgroups fit a CU (LDS 32 KB, 128 VGPRs each), i.e. 1 024 - more costs a second round (2 x on the first build, +2 % in
// the round-5 step at 1 536 / 2 048), fewer leaves matrix pipes idle.  The history of this choice (768 / 896 workgroups, an even schedule,
// unsplit segment-level gradients, tdnn1 as 128 ... 512 workgroups, wave groups) is DESIGN.md Appendix A.
struct XvTnPlan { int splits, chunk; bool wide, ahead; };      // wide: xv_gemm_tn160_kernel; ahead: TNArgs::ahead of xv_gemm_tn_kernel
static XvTnPlan xv_tn_plan(int M, int N, int R, bool direct = false) {
    const int tiles = xv_cdiv(M, BM) * xv_cdiv(N, BN);
    const int ksteps = xv_cdiv(R, BK);
    XvTnPlan pl = {1, 0, false, false};
    if (tn_wide_rows(M)) {      // xv_gemm_tn160_kernel: one round of 512 workgroups (2 per CU), at least 4 K-steps each
        const int splits = std::max(1, std::min(TNW_WGS / xv_cdiv(N, BN), ksteps / 4));
        pl.chunk = xv_cdiv(ksteps, splits) * BK;
        pl.splits = xv_cdiv(R, pl.chunk);
        pl.wide = true;         // (plain double buffering only: no `ahead` form)
        return pl;
    }
    const int min_ksteps = 2;                                          // fewest K-steps a workgroup is given
    int splits = std::max(1, XV_RESIDENT_WGS / tiles);
    if (splits > ksteps / min_ksteps) splits = std::max(1, ksteps / min_ksteps);
    // A short reduction over many tiles (the loss head's weight gradient: 232 tiles x 8 K-steps at 128 chunks) is not split: four splits of two
    // K-steps each wrote and re-read 60 MB of slabs beside the latency-bound chain of the segment layers (its d-out launch ran 45 instead of
    // 23 us); one workgroup per tile can store the result where it belongs (xv_engine_bwd.hip, loss_head_wgrad)
    // - only for the caller that asks for it (XvGemmTN::direct: its unsplit result is stored straight into the destination); a LAYER's
    // weight gradient with many tiles and a short reduction (small-batch fine-tuning) keeps its splits - unsplit it would leave most of the
    // chip idle
    if (direct && ksteps <= 16 && tiles >= 128) splits = 1;
    // A layer with few tiles (a 512 x 512 dense layer: 16) gets ONE workgroup per CU, not a co-resident round of four: 16 tiles x 16 splits =
    // 256 workgroups.  [measured, round 6, same box, alternated, profiles/r06_tn_few_tiles.txt] against 64 splits (1 024 workgroups, 67 MB of
    // slabs for a 1 MB gradient): S1 -0.4 ... -0.7 %, 64 x U{200..400} -0.1 ... -0.4 %, S2 -0.4 %, S4 -0.4 %, S5 -0.1 ... -0.4 %; alone the
    // layer's weight gradient 111.7 -> 108.4 us.  8 / 12 / 20 / 24 splits are slower than 16 (256 workgroups = the same load on every CU);
    // the same cap on the 48-tile layers (tdnn5: 21 -> 16 splits = 768 workgroups) is neutral, on the 80 / 112-tile layers harmful.
    if (tiles <= 16) splits = std::min(splits, std::max(1, 256 / tiles));
    pl.chunk = xv_cdiv(ksteps, splits) * BK;
    pl.splits = xv_cdiv(R, pl.chunk);
    pl.ahead = pl.chunk / BK >= XV_TN_AHEAD_MIN;      // (Appendix B, note 9)
    return pl;
}
int xv_tn_splits(int M, int N, int R) { return xv_tn_plan(M, N, R).splits; }
int xv_tn_splits_direct(int M, int N, int R) { return xv_tn_plan(M, N, R, true).splits; }
// diagnostics (tests/test_gemm_plans.py restates the plan against it): what xv_launch_gemm_tn runs for P[M][N] = sum over R rows
extern "C" int xv_debug_tn_plan(int M, int N, int R, int direct, int out[4]) {
    XV_REQUIRE(M > 0 && N > 0 && R > 0 && out, "debug_tn_plan: empty problem");
    const XvTnPlan pl = xv_tn_plan(M, N, R, direct != 0);
    out[0] = pl.wide ? 1 : 0;
    out[1] = pl.splits;
    out[2] = pl.chunk;
    out[3] = pl.ahead ? 1 : 0;
    return 0;
}

int xv_launch_gemm_tn(hipStream_t s, const XvGemmTN& g) {
    XV_REQUIRE(g.M % 4 == 0 && g.N % 4 == 0 && g.lda % 4 == 0 && g.ldb % 4 == 0,
               "gemm_tn: M/N/lda/ldb must be multiples of 4 (M=%d N=%d lda=%ld ldb=%ld)", g.M, g.N, g.lda, g.ldb);
    XV_REQUIRE(((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.B % 16) == 0, "gemm_tn: operands must be 16-byte aligned");
    XV_REQUIRE(g.M > 0 && g.N > 0 && g.R > 0 && g.splits >= 1, "gemm_tn: empty problem");
    TNArgs p;
    p.zero = xv_zero_page();
    if (!p.zero) return 1;
    XV_REQUIRE(g.a_rps == g.b_rps && g.a_rps > 0, "gemm_tn: both operands must share the rows-per-segment");
    XV_REQUIRE(g.R < (1 << 24), "gemm_tn: at most 2^24 reduction rows");
    {   // xv_dma16 addresses every operand row as a 32-bit byte offset from the operand's base
        const long segs = xv_cdiv(g.R, g.a_rps);
        XV_REQUIRE((segs * g.a_pitch + 1) * g.lda * 4 < (1L << 32) && (segs * g.b_pitch + 1) * g.ldb * 4 < (1L << 32),
                   "gemm_tn: an operand spans 4 GB or more (%ld segments of %d / %d rows, lda=%ld ldb=%ld): split the batch", segs, g.a_pitch,
                   g.b_pitch, g.lda, g.ldb);
    }
    p.A = g.A; p.lda = g.lda; p.a_pitch = g.a_pitch;
    p.B = g.B; p.ldb = g.ldb; p.b_pitch = g.b_pitch;
    p.rps = g.a_rps;
    // Rows without gaps between the segments (pitch == rows per segment in both operands: every dense layer, whose "segments" are single
    // frames) are ONE segment of R rows: the kernel's cheap K-step form - scalar bases, lane offsets that advance by a constant - needs
    // at least BK rows per segment, and with one-row segments every K-step took the form meant for ragged ends (a row -> address
    // resolution and a 64-bit address per lane: tdnn4 / tdnn5 ran 104 / 115 TF against 128-135 for the layers with taps; round 5).
    if (g.a_pitch == g.a_rps && g.b_pitch == g.b_rps) { p.rps = g.R; p.a_pitch = g.R; p.b_pitch = g.R; }
    p.inv_rps = 1.0f / (float)p.rps;
    p.P = g.P; p.M = g.M; p.N = g.N; p.R = g.R;
    p.tiles_m = xv_cdiv(g.M, BM); p.tiles_n = xv_cdiv(g.N, BN);
    const XvTnPlan pl = xv_tn_plan(g.M, g.N, g.R, g.direct != 0);
    XV_REQUIRE(pl.splits == g.splits, "gemm_tn: splits must come from xv_tn_splits%s (%d vs %d)", g.direct ? "_direct" : "", pl.splits, g.splits);
    p.r_chunk = pl.chunk;
    p.ahead = pl.ahead ? 1 : 0;
    const int wgs = p.tiles_m * p.tiles_n * pl.splits;
    {
        XvProfScope prof(s, 2, 2.0 * g.M * g.N * g.R);
        if (pl.wide) hipLaunchKernelGGL(xv_gemm_tn160_kernel, dim3(p.tiles_n * pl.splits), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(xv_gemm_tn_kernel, dim3(wgs), dim3(256), 0, s, p);
    }
    XV_LAUNCH_CHECK();
    return 0;
}

// -------------------------------------------------------------------------------------
// Public op-level wrappers around the two GEMMs
// -------------------------------------------------------------------------------------
extern "C" size_t xv_op_workspace_bytes(int rows, int cols_in, int cols_out) {
    // split slabs: at most XV_RESIDENT_WGS (+ one ragged round) workgroup tiles of 128x128 floats, plus column partials
    size_t slabs = (size_t)(2 * XV_RESIDENT_WGS + 256) * BM * BN * sizeof(float);      // NT: two shared tiles per workgroup; TN: two segments
    size_t wg = (size_t)xv_align(cols_in, BM) * xv_align(cols_out, BN) * sizeof(float) * 8;
    size_t part = ((size_t)xv_cdiv(rows > 0 ? rows : 1, 64) * 2 + 2) * (size_t)(cols_out > cols_in ? cols_out : cols_in) * sizeof(float);
    size_t m = slabs > wg ? slabs : wg;
    return xv_align((m > part ? m : part) + 4096, 256);
}

// out[(j*C + c)][n] = sum_z P[z][j*c_pad + c][n] (+ l2 * w[(j*C + c)][n])
// Block = 64 column quads (16 B per lane) x 4; splits are added in split order with eight loads in flight.  ZSPLIT (many splits, few
// output rows - tdnn1: 150 rows x 128 splits): the 4 thread groups of a block take contiguous runs of the splits of ONE row and their sums
// are added in group order (a fixed association: bit-reproducible).  Otherwise the 4 groups are 4 rows and a thread adds all splits of
// its quad.  Row blocks are grid-strided (at most ~2 048 workgroups: a launch of many short workgroups crawls beside a GEMM).
// (The first build read 4 bytes per lane with two 64-bit divisions per element: 45 us for tdnn2's 63 MB of slabs alone on the chip -
// and the last of these launches sits between the last GEMM of a step and the update.)
#define WR_FLIGHT 8
template <bool ZSPLIT>
__global__ __launch_bounds__(256) void xv_wgrad_reduce_kernel(const float* __restrict__ P, int splits, long slab, int rows, int C, int c_pad,
                                                              int n_in, int nq_out, const float* __restrict__ w, long ldw, float l2,
                                                              float* __restrict__ out, long ldo) {
    XV_EW_PRIORITY();
    __shared__ f32x4 part[ZSPLIT ? 4 : 1][64];
    const int qx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + qx;
    const bool qv = q < nq_out;
    const int per = ZSPLIT ? (splits + 3) / 4 : splits;
    const int z0 = ZSPLIT ? g * per : 0, z1 = min(splits, z0 + per);
    for (int rb = blockIdx.y; rb * (ZSPLIT ? 1 : 4) < rows; rb += gridDim.y) {
        const int row = ZSPLIT ? rb : 4 * rb + g;
        const bool rv = row < rows;
        const int rr = rv ? row : 0;
        const int j = rr / C, c = rr - j * C;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qv && rv) {
            const float* src = P + ((long)j * c_pad + c) * n_in + 4 * q;
            for (int z = z0; z < z1; z += WR_FLIGHT) {
                f32x4 t[WR_FLIGHT];
#pragma unroll
                for (int u = 0; u < WR_FLIGHT; ++u) t[u] = *(const f32x4*)(src + (long)min(z + u, z1 - 1) * slab);
#pragma unroll
                for (int u = 0; u < WR_FLIGHT; ++u)
                    if (z + u < z1) v += t[u];
            }
        }
        if (ZSPLIT) {
            __syncthreads();      // (the previous row's sums have been read)
            part[g][qx] = v;
            __syncthreads();
            if (g != 0) continue;
            v = ((part[0][qx] + part[1][qx]) + part[2][qx]) + part[3][qx];
        }
        if (qv && rv) {
            if (w) v += l2 * *(const f32x4*)(w + (long)row * ldw + 4 * q);
            *(f32x4*)(out + (long)row * ldo + 4 * q) = v;
        }
    }
}

int xv_launch_wgrad_reduce(hipStream_t s, const float* P, int splits, int k, int C, int c_pad, int n_in, int n_out, const float* w,
                           long ldw, float l2, float* out, long ldo) {
    XV_REQUIRE(n_out % 4 == 0 && n_in % 4 == 0 && ldo % 4 == 0 && (!w || ldw % 4 == 0) && ((uintptr_t)P % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                   (!w || ((uintptr_t)w % 16) == 0),
               "wgrad_reduce: widths and leading dimensions must be multiples of 4 floats, buffers 16-byte aligned (n_out=%d)", n_out);
    const int rows = k * C, gx = xv_cdiv(n_out / 4, 64);
    const bool zsplit = splits >= 32 && (long)rows * gx < 1024;
    const int row_blocks = zsplit ? rows : xv_cdiv(rows, 4);
    const dim3 grid(gx, std::min(row_blocks, std::max(1, 2048 / gx)));      // (256 ... 4 096: no difference in the step, profiles/r06_tn_few_tiles.txt)
    if (zsplit)
        hipLaunchKernelGGL(xv_wgrad_reduce_kernel<true>, grid, dim3(256), 0, s, P, splits, (long)k * c_pad * n_in, rows, C, c_pad, n_in, n_out / 4, w,
                           ldw, l2, out, ldo);
    else
        hipLaunchKernelGGL(xv_wgrad_reduce_kernel<false>, grid, dim3(256), 0, s, P, splits, (long)k * c_pad * n_in, rows, C, c_pad, n_in, n_out / 4, w,
                           ldw, l2, out, ldo);
    XV_LAUNCH_CHECK();
    return 0;
}

int xv_affine_wgrad_ld(hipStream_t stream, const float* x, int segs, int t_in, int c_pad, int k, int c, const float* dz, int ldo, int dz_seg_pitch,
                       int dz_row0, int o, const float* kernel, float l2_scale, float* dkernel, void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_in >= k && c_pad >= c && o > 0 && o % 4 == 0 && ldo >= o && ldo % 4 == 0,
               "affine_wgrad: bad shape (o=%d must be a multiple of 4)", o);
    const int t_out = t_in - k + 1;
    XvGemmTN g = {};
    g.A = x; g.lda = c_pad; g.a_rps = t_out; g.a_pitch = t_in;
    g.B = dz + (long)dz_row0 * ldo; g.ldb = ldo; g.b_rps = t_out; g.b_pitch = dz_seg_pitch;
    g.M = k * c_pad; g.N = o; g.R = segs * t_out;
    g.splits = xv_tn_splits(g.M, g.N, g.R);
    XV_REQUIRE((size_t)g.splits * g.M * g.N * sizeof(float) <= ws_bytes, "affine_wgrad: workspace too small (%zu needed)",
               (size_t)g.splits * g.M * g.N * sizeof(float));
    g.P = (float*)ws;
    int rc = xv_launch_gemm_tn(stream, g);
    if (rc) return rc;
    return xv_launch_wgrad_reduce(stream, g.P, g.splits, k, c, c_pad, o, o, l2_scale != 0.f ? kernel : nullptr, o,
                                  l2_scale, dkernel, o);
}
extern "C" int xv_affine_wgrad(void* stream, const float* x, int segs, int t_in, int c_pad, int k, int c, const float* dz,
                               int dz_seg_pitch, int dz_row0, int o, const float* kernel, float l2_scale, float* dkernel, void* ws,
                               size_t ws_bytes) {
    return xv_affine_wgrad_ld((hipStream_t)stream, x, segs, t_in, c_pad, k, c, dz, o, dz_seg_pitch, dz_row0, o, kernel, l2_scale, dkernel, ws, ws_bytes);
}
