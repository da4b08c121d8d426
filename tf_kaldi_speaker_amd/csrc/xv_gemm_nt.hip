// fp32 MFMA GEMM, "NT" shape, for the TDNN hot path (gfx950 / CDNA4 only):
//
//  NT  C[m][n] = sum_k A[rowmap(m)][k] * Bt[n][k]
//      forward conv/dense (A = spliced activation view, Bt = kernel^T), data gradients
//      (A = zero-padded dz view, Bt = tap-flipped kernel), logits.
//
// (The other shape of tdnn.py / loss.py, the weight gradients' reduction over rows, is xv_gemm_tn.hip.)  Here: the one-workgroup-per-tile
// kernel, the evenly scheduled kernel, the split-K slab sum, the planner and launcher, the zero page and the ticket pool, and the
// xv_affine_forward / xv_affine_dgrad entry points.  The device pieces both kernels share are stated once in xv_gemm_tile.h.
//
// The "spliced view" makes the context window free: row (b,t) of a layer with context k is
// the contiguous span x[b][t..t+k-1][:], so rowmap(m) = (m / rps) * pitch + (m % rps) with
// leading dimension C < K.  Rows overlap in memory; the 128-row A tile of one workgroup
// therefore re-reads the same (128+k-1) x C window k times from L2, never from HBM.
//
// Both kernels (and the TN kernel): 128x128 output tile, 256 threads = 4 waves (2x2), each wave a 64x64 sub-tile
// as 2x2 v_mfma_f32_32x32x2_f32 accumulators (64 acc VGPRs), K-step XV_TILE_K = 16, operand tiles
// staged by LDS-DMA (global_load_lds_dwordx4, scalar base + 32-bit lane offsets: xv_dma16 in xv_handoff.h - the address
// form decides what a stage costs the MFMA pipe) into a double-buffered 32 KB LDS image (xv_gemm_tile.h), one barrier per K-step,
// XV_WGS_PER_CU = 4 workgroups per CU (xv_gemm.h).
//
// MFMA operand maps (cdna_hip_programming.md section 3): lane l supplies A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; D register r of lane l is row (r&3)+8*(r>>2)+4*(l>>5), column l&31.
// The contraction is order-insensitive in k as long as A and B agree, so the NT kernel lets
// lane-half h own 4 CONSECUTIVE k of every 8 (one ds_read_b128 feeds 4 MFMAs).
#include "xv_common.h"
#include "xv_gemm.h"
#include "xv_gemm_tile.h"
#include "xv_epilogue.h"
#include "xv_diag.h"
#include <algorithm>
#include <map>
#include <mutex>

#define BM XV_TILE_M
#define BN XV_TILE_N
#define BK XV_TILE_K

struct NTArgs {
    const float* A; long lda; int a_rps; int a_pitch;
    const float* Bt; long ldb;
    float* C; long ldc; long c_split_stride;
    int M, N, K, k_chunk;
    int tiles_m, tiles_n;
    const float* bias;
    float* part_sum; float* part_m2;
    const float* zero;
    int stamp_half;      // diagnostics build only (xv_diag.h): the stamp buffer half of this launch, -1 = none
    // "whole tiles + shares" (xv_launch_gemm_nt): blocks [0, n_whole) take one whole tile each; the tiles behind them are cut into `shares`
    // equal K ranges, one block each (grid = n_whole + (tiles - n_whole) * shares); shares <= 1: every block a whole tile
    int n_whole, shares;
    float* slab;                // [(tiles - n_whole) * shares][128 * 128]: partial tiles in lane order
    unsigned* tickets;          // one per tile, zero between launches
    int row_store;              // epilogue through LDS with 16-byte row stores (nt_store_tile_rows): C / ldc 16-byte aligned, N % 4 == 0
};

// Out-of-range rows / k read this 16-byte zero page instead of being masked after the load: the
// select is on the ADDRESS, so every global_load is unconditional and hipcc neither branches
// around it nor drains vmcnt right behind it (the first build waited vmcnt(0) four times per
// K-step at the top of the loop: profiles/r01_first_bench.json, 53 % of the MFMA roof).
// The page is ordinary hipMalloc'd global memory handed in through the kernel arguments (a
// __device__ constant made the selected pointer generic -> flat_load, which also counts on
// lgkmcnt and so serialised the LDS fragment reads behind the global loads).
// The page is XV_ZERO_PAGE_FLOATS long: an out-of-range ROW is redirected to it ONCE (its base pointer), after which "base + k"
// stays inside the page for every k < K <= XV_ZERO_PAGE_FLOATS - so full K-steps stage with no per-step select at all.
static float* g_zero_page = nullptr;
static size_t g_zero_page_floats = 0;
// Grows on demand (a reduction longer than the page, e.g. the gradient through a 20 000-speaker loss head: K = the speaker count).
// The old page is left alive: launches already enqueued may still read it, and a page is a few hundred KB at most.
static int ensure_zero_page(size_t floats = XV_ZERO_PAGE_FLOATS) {
    if (g_zero_page && floats <= g_zero_page_floats) return 0;
    size_t want = XV_ZERO_PAGE_FLOATS;
    while (want < floats) want *= 2;
    float* p = nullptr;
    XV_CHECK_HIP(hipMalloc((void**)&p, want * sizeof(float)));
    XV_CHECK_HIP(hipMemset(p, 0, want * sizeof(float)));
    g_zero_page = p;
    g_zero_page_floats = want;
    return 0;
}
const float* xv_zero_page(size_t floats) { return ensure_zero_page(floats) ? nullptr : g_zero_page; }

// (What did and did not move this kernel's K loop: DESIGN.md Appendix B, note 2.)
template <bool STATS, bool ROWS>
__global__ __launch_bounds__(256, XV_WGS_PER_CU) __attribute__((amdgpu_num_vgpr(128))) void xv_gemm_nt_kernel(NTArgs p) {
    __shared__ __attribute__((aligned(16))) float smem[2 * 2 * BM * NT_PITCH];      // two slots of [A | B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    XV_STAMP_ENTRY(p.stamp_half);
    unsigned long long stall = 0;
    (void)stall;

    // whole tiles first: the hardware places them first (n_whole is a multiple of 256 - the same number on every CU of an empty chip), the
    // short share blocks behind them are dealt into whatever slots are free
    const bool shared = p.shares > 1 && (int)blockIdx.x >= p.n_whole;      // (uniform)
    int t, share = 0;
    if (p.shares > 1) {
        if (shared) {
            const int r = xcd_swizzle(blockIdx.x - p.n_whole, gridDim.x - p.n_whole);      // (n_whole % 8 == 0: the XCD of a block is blockIdx % 8 in both ranges)
            t = p.n_whole + r / p.shares;
            share = r - (r / p.shares) * p.shares;
        } else {
            t = xcd_swizzle(blockIdx.x, p.n_whole);
        }
    } else {
        t = xcd_swizzle(blockIdx.x, gridDim.x);
    }
    const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    int k_begin = blockIdx.z * p.k_chunk;
    int k_end = min(p.K, k_begin + p.k_chunk);
    if (shared) {      // share i of a tile: K-steps [i * nk / shares, (i + 1) * nk / shares)
        const int nk_tile = (p.K + BK - 1) / BK;
        k_begin = (int)((long)share * nk_tile / p.shares) * BK;
        k_end = min(p.K, (int)((long)(share + 1) * nk_tile / p.shares) * BK);
    }
    // (uniform by construction; said explicitly because xv_dma16 takes "operand base + k" in SGPRs - the diagnostics build otherwise keeps
    // the share arithmetic in vector registers and the assembler rejects the DMA)
    k_begin = __builtin_amdgcn_readfirstlane(k_begin);
    k_end = __builtin_amdgcn_readfirstlane(k_end);
    const int nk = (k_end - k_begin + BK - 1) / BK;

    // ---- global -> LDS staging by LDS-DMA (global_load_lds_dwordx4): no staging VGPRs, no ds_write.
    // One wave-instruction writes 1 KiB linearly (wave-uniform base + lane*16 B) = NT_RPI whole tile rows,
    // so lane l lands on row RPI*(RPT*wave+i) + l/KQ at chunk POSITION l%KQ; the XOR swizzle therefore
    // moves to the SOURCE: that lane fetches chunk (l%KQ) ^ f(row) of its row (rule: swizzle source +
    // read, never the DMA destination).  Out-of-range rows / k fetch the zero page.
    constexpr int NT_RPI = 64 / NT_KQ;          // tile rows per wave-instruction (16 at BK=16)
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int lrow = lane / NT_KQ, lpos = lane % NT_KQ;
    // per-lane byte offsets from p.A / p.Bt with the swizzled chunk folded in (xv_dma16: scalar base + 32-bit offset).  Rows outside the
    // matrix read row 0 - their products land in accumulator rows / columns that are neither stored nor counted; only k beyond k_end must
    // read zeros (it is summed into valid outputs): the ragged last K-step takes the zero page through the builtin's 64-bit form.
    const float* __restrict__ zp = p.zero;
    unsigned aoff[NT_RPT], boff[NT_RPT];
    int ksrc[NT_RPT];
#pragma unroll
    for (int i = 0; i < NT_RPT; ++i) {
        int row = NT_RPI * (NT_RPT * wave + i) + lrow;
        ksrc[i] = ((lpos ^ NT_SWZ(row)) << 2);
        int m = m0 + row;
        int mm = m < p.M ? m : 0;
        int seg = mm / p.a_rps, tt = mm - seg * p.a_rps;
        aoff[i] = (unsigned)((((long)seg * p.a_pitch + tt) * p.lda + ksrc[i]) * 4);
        int n = n0 + row;
        boff[i] = (unsigned)(((long)(n < p.N ? n : 0) * p.ldb + ksrc[i]) * 4);
    }
    const unsigned lds0 = xv_lds_addr(smem + NT_RPI * NT_RPT * uwave * NT_PITCH);
    auto gstage = [&](int kt, int buf) {
        const int k0 = k_begin + kt * BK;
        if (k0 + BK <= k_end) {        // full K-step (uniform): scalar bases + k0, the lane offsets never change
            const float* abase = p.A + k0;
            const float* bbase = p.Bt + k0;
#pragma unroll
            for (int i = 0; i < NT_RPT; ++i) {
                xv_dma16(abase, aoff[i], lds0 + (buf * (2 * BM * NT_PITCH) + NT_RPI * i * NT_PITCH) * 4);
                xv_dma16(bbase, boff[i], lds0 + (buf * (2 * BM * NT_PITCH) + BM * NT_PITCH + NT_RPI * i * NT_PITCH) * 4);
            }
        } else {                       // ragged last step: chunks at or beyond k_end come from the zero page
            float* sa = smem + buf * (2 * BM * NT_PITCH) + NT_RPI * NT_RPT * uwave * NT_PITCH;
            float* sb = sa + BM * NT_PITCH;
#pragma unroll
            for (int i = 0; i < NT_RPT; ++i) {
                const bool kv = k0 + ksrc[i] < k_end;
                const float* pa = (const float*)((const char*)(p.A + k0) + aoff[i]);
                const float* pb = (const float*)((const char*)(p.Bt + k0) + boff[i]);
                xv_dma16_ptr((kv ? pa : zp), sa + NT_RPI * i * NT_PITCH);
                xv_dma16_ptr((kv ? pb : zp), sb + NT_RPI * i * NT_PITCH);
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int a_off = (wr * 64 + li) * NT_PITCH;
    const int b_off = (wc * 64 + li) * NT_PITCH;
    const int fsw = NT_SWZ(li);     // rows wr*64 + a*32 + li share f(li): the offsets are multiples of 16
    if (nk > 0) gstage(0, 0);
    xv_dma_wait_all();
    __syncthreads();
    XV_STAMP(p.stamp_half, 1);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gstage(kt + 1, buf ^ 1);
        const float* sa = smem + buf * (2 * BM * NT_PITCH);
        const float* sb = sa + BM * NT_PITCH;
#pragma unroll
        for (int q = 0; q < BK / 8; ++q) {
            f32x4 af[2], bf[2];
            const int pos = (((2 * q + lh) ^ fsw) << 2);
            af[0] = *(const f32x4*)(sa + a_off + pos);
            af[1] = *(const f32x4*)(sa + a_off + 32 * NT_PITCH + pos);
            bf[0] = *(const f32x4*)(sb + b_off + pos);
            bf[1] = *(const f32x4*)(sb + b_off + 32 * NT_PITCH + pos);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0][e], bf[0][e], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0][e], bf[1][e], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1][e], bf[0][e], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1][e], bf[1][e], acc[1][1], 0, 0, 0);
            }
        }
        xv_dma_wait_all();      // the compiler does not see xv_dma16's loads
        XV_DIAG_BARRIER(stall);
    }
    XV_STAMP(p.stamp_half, 2);

    bool alive = true;
    if (shared) {
        // a share of a tile: publish it (lane-order slab: 1 KB of consecutive bytes per wave instruction), take the tile's ticket, and only
        // the last of the tile's blocks goes on: it sums the shares in K order - ((s0 + s1) + s2) + ... whoever it is; the first two commute,
        // so a block that holds share 0 or 1 keeps it in registers - and runs the ordinary epilogue (xv_handoff_* contract, xv_handoff.h)
        int& s_last = *(int*)smem;      // (the staging buffers are idle)
        const int first = (t - p.n_whole) * p.shares;
        float* mine = p.slab + (long)(first + share) * (BM * BN) + tid * 4;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x4 v = {acc[0][0][r], acc[0][1][r], acc[1][0][r], acc[1][1][r]};
            xv_handoff_store4(mine + r * (256 * 4), v);
        }
        xv_handoff_drain();
        __syncthreads();
        if (tid == 0) s_last = xv_ticket_take(p.tickets + t, (unsigned)p.shares) ? 1 : 0;
        __syncthreads();
        const int last = s_last;
        __syncthreads();                // (s_last aliases the scratch the statistics use below)
        alive = last != 0;              // (uniform) the other shares of the tile are done
        if (alive && share > 1) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        }
        for (int i = 0; alive && i < p.shares; ++i) {
            const int v = share == 1 ? (i == 0 ? 1 : i == 1 ? 0 : i) : i;      // share 1: own, share 0, share 2, ...
            if (v == share && share <= 1) continue;
            const float* src = p.slab + (long)(first + v) * (BM * BN) + tid * 4;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 x[8];
                xv_handoff_load8(src + 8 * h * (256 * 4), 256 * 4, x);
#pragma unroll
                for (int k8 = 0; k8 < 8; ++k8) {
                    const int r = 8 * h + k8;
                    acc[0][0][r] += x[k8][0]; acc[0][1][r] += x[k8][1]; acc[1][0][r] += x[k8][2]; acc[1][1][r] += x[k8][3];
                }
            }
        }
    }
    // ---- epilogue
    if (alive) {
        float* C = p.C + (long)blockIdx.z * p.c_split_stride;
        if (ROWS) nt_store_tile_rows(acc, smem, C, p.ldc, p.bias, m0, n0, p.M, p.N, tid, wr, wc, li, lh);
        else nt_store_tile(acc, C, p.ldc, p.bias, m0, n0, p.M, p.N, wr, wc, li, lh);
        if (STATS) xv_tile_stats_epilogue(acc, smem, tid, wr, wc, li, lh, m0, n0, p.M, p.N, tile_m, p.tiles_m, p.part_sum);
    }
    XV_STAMP_EXIT(p.stamp_half, stall);
}

// -------------------------------------------------------------------------------------
// NT, evenly scheduled ("stream-K"): the launch has P persistent workgroups (one co-resident round) and every one of them runs the
// same number of K-steps.  The (tile, K-step) pairs are numbered tile-major, u = tile * nk + kt; workgroup w owns the units
// [w * total / P, (w + 1) * total / P) - a run that may start and end in the middle of a tile.  A tile whose K-steps were shared
// stores its partial accumulators as slabs (the lane-order layout of the TN kernel), and the workgroup that finishes its share
// LAST sums them in K order (xv_handoff_* contract) and runs the ordinary epilogue (bias, store, BatchNorm statistics).
// It exists for tile-count quantisation (784 tiles on 768 slots, 2.3 tiles per CU in the shipped batch): DESIGN.md Appendix B, note 3.
struct NTSKArgs {
    NTArgs g;
    int P;                    // workgroups (grid size)
    int nk;                   // K-steps per tile
    long total;               // tiles * nk
    float* slab;              // [P][2][128*128]: first / last partial tile of each workgroup
    unsigned* tickets;        // one per tile, zero between launches
};

__device__ __forceinline__ int ntsk_owner(long u, int P, long total) { return (int)((((u + 1) * P) - 1) / total); }

// (Its context-window form of rounds 2-4 - the rows of one 16-channel chunk of x staged once for all taps - is gone: DESIGN.md Appendix B, note 4.)
#define XV_NT_SK_WPC 3                       // workgroups per CU of the even schedule: one co-resident round of 768 (2 / 4 per CU: S1 +0.5 %, round 6)
// Register budget: 128 VGPRs (4 waves per SIMD) although the launch is 3 workgroups per CU - the free fourth slot is worth more to the other
// stream than the 7-23 spilled set-up registers cost (note 5; tools/variant.sh unit xv_gemm_nt.hip "sk168:-DXV_NT_SK_VGPRS=168 -DXV_NT_SK_OCC=3").
#ifndef XV_NT_SK_VGPRS
#define XV_NT_SK_VGPRS 128
#define XV_NT_SK_OCC XV_WGS_PER_CU
#endif
template <bool STATS, bool ROWS>
__global__ __launch_bounds__(256, XV_NT_SK_OCC) __attribute__((amdgpu_num_vgpr(XV_NT_SK_VGPRS))) void xv_gemm_nt_sk_kernel(NTSKArgs q) {
    const NTArgs& p = q.g;
    constexpr int A_SLOT = BM * NT_PITCH;       // floats per A slot
    constexpr int B_SLOT = BM * NT_PITCH;
    __shared__ __attribute__((aligned(16))) float smem[2 * A_SLOT + 2 * B_SLOT];   // [A slot 0 | A slot 1 | B slot 0 | B slot 1]
    int& s_last = *(int*)smem;      // (the staging buffers are idle when it is used)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int w = xcd_swizzle(blockIdx.x, gridDim.x);
    // (unit indices fit 32 bits - the launcher checks total < 2^31 -; as 64-bit scalars they were five register pairs live across the whole run)
    const int u_end = (int)((long)(w + 1) * q.total / q.P);
    int u = (int)((long)w * q.total / q.P);
    const int first_tile = (int)(u / q.nk);
    XV_STAMP_ENTRY(p.stamp_half);
    bool first_seg = true;
    (void)first_seg;

    constexpr int NT_RPI = 64 / NT_KQ;          // tile rows per wave-instruction (16 at BK=16)
    const int uwave = __builtin_amdgcn_readfirstlane(wave);
    const int lrow = lane / NT_KQ, lpos = lane % NT_KQ;
    const float* __restrict__ zp = p.zero;
    const int b_off = (wc * 64 + li) * NT_PITCH;
    const int fsw = NT_SWZ(li);
    const int wslot = xv_wave_slot();
    // LDS byte addresses this wave's DMA pieces land at (slot 0; xv_dma16)
    const unsigned lds_a = xv_lds_addr(smem + NT_RPI * NT_RPT * uwave * NT_PITCH);
    const unsigned lds_b = xv_lds_addr(smem + 2 * A_SLOT + NT_RPI * NT_RPT * uwave * NT_PITCH);

    // Order of a run that ends one tile and begins the next ([k0, nk) of tile t, then [0, k2) of tile t + 1): the BEGINNING of the next tile
    // first.  Every workgroup then walks K upwards from (about) 0 in step with the others, so the K-slices of the weight matrix in flight on
    // an XCD at any moment are the same few for all its workgroups, as in a one-workgroup-per-tile launch.  In run order the workgroups of
    // an XCD sit at all K offsets at once, their weight slices do not fit the L2 together and are re-fetched from the Infinity Cache
    // (1.45 -> 0.16 GB past the L2 per launch, same time: DESIGN.md Appendix B, note 6.)
    const int u_begin = u;
    const int u_mid = (u / q.nk + 1) * q.nk;                   // end of the first tile of the run
    const bool wrap_first = u % q.nk != 0 && u_mid < u_end && u_end - u_mid <= q.nk;
    for (int pass = 0; pass < 2; ++pass) {
    int u_stop = u_end;
    if (wrap_first) { u = pass == 0 ? u_mid : u_begin; u_stop = pass == 0 ? u_end : u_mid; }
    else if (pass == 1) break;
    while (u < u_stop) {
        const int tile = (int)(u / q.nk);
        const int kt0 = u - tile * q.nk;
        const int kt1 = min(q.nk, kt0 + (u_stop - u));
        const int tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
        const int m0 = tile_m * BM, n0 = tile_n * BN;

        // per-lane byte offsets of this tile from p.A / p.Bt (swizzled chunk folded in; xv_dma16).  Rows outside the operand read row 0:
        // their products only reach accumulator rows / columns that are never stored, counted or - in a shared tile - used after the sum
        unsigned aoff[NT_RPT];
        unsigned boff[NT_RPT];
        int ksrc[NT_RPT];
        int a_row[2];                           // LDS offsets of this lane's two fragment rows
        // (the ragged last K-step of a row needs each piece's k offset again: rebuilt from the hardware lane index there, not kept in a register)
        auto ksrc_now = [&](int i) {
            const int l = xv_lane_id();
            return (((l % NT_KQ) ^ NT_SWZ(NT_RPI * (NT_RPT * uwave + i) + l / NT_KQ)) << 2);
        };
#pragma unroll
        for (int i = 0; i < NT_RPT; ++i) {
            const int row = NT_RPI * (NT_RPT * wave + i) + lrow;
            ksrc[i] = ((lpos ^ NT_SWZ(row)) << 2);
            const int n = n0 + row;
            boff[i] = (unsigned)(((long)(n < p.N ? n : 0) * p.ldb + ksrc[i]) * 4);
        }
        {
#pragma unroll
            for (int i = 0; i < NT_RPT; ++i) {
                const int row = NT_RPI * (NT_RPT * wave + i) + lrow;
                const int m = m0 + row;
                const int mm = m < p.M ? m : 0;
                const int seg = mm / p.a_rps, tt = mm - seg * p.a_rps;
                aoff[i] = (unsigned)((((long)seg * p.a_pitch + tt) * p.lda + ksrc[i]) * 4);
            }
            a_row[0] = (wr * 64 + li) * NT_PITCH;
            a_row[1] = a_row[0] + 32 * NT_PITCH;
        }
        // K-step kt of a tile = columns [kt*BK, +BK) of the spliced row
        // (A and B apart and `ksrc_now` instead of a kept register - xv_gemm_nt_kernel stages A and B pairwise from ksrc[]: the forms differ
        // in order and registers on purpose, so there is no shared staging function)
        auto stage_b = [&](int kt, int slot) {
            const int k0 = kt * BK;
            if (k0 + BK <= p.K) {
                const float* bbase = p.Bt + k0;
#pragma unroll
                for (int i = 0; i < NT_RPT; ++i) xv_dma16(bbase, boff[i], lds_b + (slot * B_SLOT + NT_RPI * i * NT_PITCH) * 4);
            } else {                       // ragged last step of a row: chunks at or beyond K come from the zero page
                float* sb = smem + 2 * A_SLOT + slot * B_SLOT + NT_RPI * NT_RPT * uwave * NT_PITCH;
#pragma unroll
                for (int i = 0; i < NT_RPT; ++i) {
                    const float* pb = (const float*)((const char*)(p.Bt + k0) + boff[i]);
                    xv_dma16_ptr((k0 + ksrc_now(i) < p.K ? pb : zp), sb + NT_RPI * i * NT_PITCH);
                }
            }
        };
        auto stage_a = [&](int kt, int slot) {      // the tile's rows of K-step kt
            const int k0 = kt * BK;
            if (k0 + BK <= p.K) {          // full K-step (uniform): scalar base + k0, the lane offsets never change
                const float* abase = p.A + k0;
#pragma unroll
                for (int i = 0; i < NT_RPT; ++i) xv_dma16(abase, aoff[i], lds_a + (slot * A_SLOT + NT_RPI * i * NT_PITCH) * 4);
            } else {
                float* sa = smem + slot * A_SLOT + NT_RPI * NT_RPT * uwave * NT_PITCH;
#pragma unroll
                for (int i = 0; i < NT_RPT; ++i) {
                    const float* pa = (const float*)((const char*)(p.A + k0) + aoff[i]);
                    xv_dma16_ptr((k0 + ksrc_now(i) < p.K ? pa : zp), sa + NT_RPI * i * NT_PITCH);
                }
            }
        };

        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

        stage_a(kt0, 0);
        stage_b(kt0, 0);
        xv_dma_wait_all();      // (the compiler does not see xv_dma16's loads)
        __syncthreads();
        XV_STAMP_ONCE(p.stamp_half, 1, first_seg);
        for (int kt = kt0; kt < kt1; ++kt) {
            const int buf = (kt - kt0) & 1;
            xv_rot_prio(kt + wslot);
            if (kt + 1 < kt1) {
                stage_a(kt + 1, buf ^ 1);
                stage_b(kt + 1, buf ^ 1);
            }
            const float* sa = smem + buf * A_SLOT;
            const float* sb = smem + 2 * A_SLOT + buf * B_SLOT;
            // (the K-step of xv_gemm_nt_kernel, written out: as a shared function it changes both kernels' instruction order - xv_gemm_tile.h)
#pragma unroll
            for (int qq = 0; qq < BK / 8; ++qq) {
                f32x4 af[2], bf[2];
                const int pos = (((2 * qq + lh) ^ fsw) << 2);
                af[0] = *(const f32x4*)(sa + a_row[0] + pos);
                af[1] = *(const f32x4*)(sa + a_row[1] + pos);
                bf[0] = *(const f32x4*)(sb + b_off + pos);
                bf[1] = *(const f32x4*)(sb + b_off + 32 * NT_PITCH + pos);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0][e], bf[0][e], acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[0][e], bf[1][e], acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1][e], bf[0][e], acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[1][e], bf[1][e], acc[1][1], 0, 0, 0);
                }
            }
            xv_dma_wait_all();
            __syncthreads();
        }
        u += kt1 - kt0;
        __builtin_amdgcn_s_setprio(0);
        XV_STAMP(p.stamp_half, 2);

        if (kt0 != 0 || kt1 != q.nk) {
            // a shared tile: publish this share, take a ticket, and only the last of the tile's workgroups goes on
            // slab of a share: [register r][thread] float4 = (acc[0][0][r], acc[0][1][r], acc[1][0][r], acc[1][1][r]): 1 KB of consecutive
            // bytes per wave instruction, stores and loads alike
            const int tid_h = uwave * 64 + xv_lane_id();      // (rebuilt: keeps the slab addresses out of the registers that live across the K loop)
            // (publish and accumulate as in xv_gemm_nt_kernel, written out in both: shared functions change the instruction order - xv_gemm_tile.h)
            float* mine = q.slab + ((long)w * 2 + (tile == first_tile ? 0 : 1)) * (BM * BN) + tid_h * 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 v = {acc[0][0][r], acc[0][1][r], acc[1][0][r], acc[1][1][r]};
                xv_handoff_store4(mine + r * (256 * 4), v);
            }
            xv_handoff_drain();
            __syncthreads();
            const long t_first = (long)tile * q.nk;
            const int w_first = ntsk_owner(t_first, q.P, q.total), w_last = ntsk_owner(t_first + q.nk - 1, q.P, q.total);
            if (tid == 0) s_last = xv_ticket_take(q.tickets + tile, (unsigned)(w_last - w_first + 1)) ? 1 : 0;
            __syncthreads();
            const int last = s_last;                     // s_last aliases the staging buffers: every wave has read it before the barrier
            __syncthreads();                             // below lets anyone stage the next share or use the statistics scratch
            if (!last) continue;                         // (uniform)
            // The tile's value is ((s0 + s1) + s2) + ... in K order whoever arrives last.  The first two shares commute, so a workgroup that
            // holds share 0 or 1 keeps it in its registers and reads only the others (one slab for the usual two-share tile); a later
            // share is re-read from its slab at its place in the order.
            const int me = w - w_first;
            if (me > 1) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
            }
            for (int i = 0; i <= w_last - w_first; ++i) {
                const int v = w_first + (me == 1 ? (i == 0 ? 1 : i == 1 ? 0 : i) : i);      // me == 1: own, share 0, share 2, ...
                if (v == w && me <= 1) continue;
                const int v_first_tile = (int)(((long)v * q.total / q.P) / q.nk);
                const float* src = q.slab + ((long)v * 2 + (tile == v_first_tile ? 0 : 1)) * (BM * BN) + tid_h * 4;
                // eight 16-byte loads in flight per lane: a shared tile end is a latency chain (four in flight: no scratch, step +1.5 %; DESIGN.md Appendix B, note 7)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4 x[8];
                    xv_handoff_load8(src + 8 * h * (256 * 4), 256 * 4, x);
#pragma unroll
                    for (int k8 = 0; k8 < 8; ++k8) {
                        const int r = 8 * h + k8;
                        acc[0][0][r] += x[k8][0]; acc[0][1][r] += x[k8][1]; acc[1][0][r] += x[k8][2]; acc[1][1][r] += x[k8][3];
                    }
                }
            }
        }
        const int lane_e = xv_lane_id(), tid_e = uwave * 64 + lane_e, wr_e = uwave >> 1, wc_e = uwave & 1, li_e = lane_e & 31, lh_e = lane_e >> 5;
        if (ROWS) nt_store_tile_rows(acc, smem, p.C, p.ldc, p.bias, m0, n0, p.M, p.N, tid_e, wr_e, wc_e, li_e, lh_e);
        else nt_store_tile(acc, p.C, p.ldc, p.bias, m0, n0, p.M, p.N, wr_e, wc_e, li_e, lh_e);
        if (STATS) {
            xv_tile_stats_epilogue(acc, smem, tid_e, wr_e, wc_e, li_e, lh_e, m0, n0, p.M, p.N, tile_m, p.tiles_m, p.part_sum);
            __syncthreads();                             // the statistics use the staging buffers as scratch
        }
    }
    }
    XV_STAMP_EXIT(p.stamp_half, 0);
}

// out[m][n] = sum_z slab[z][m][n] (+ bias[n])
__global__ void xv_splitk_reduce_kernel(const float* __restrict__ slab, int splits, long split_stride, int M, int N,
                                        int lds, const float* __restrict__ bias, float* __restrict__ out, long ldo) {
    XV_EW_PRIORITY();
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)M * N;
    for (; idx < total; idx += (long)gridDim.x * blockDim.x) {
        int m = (int)(idx / N), n = (int)(idx - (long)m * N);
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += slab[z * split_stride + (long)m * lds + n];
        if (bias) v += bias[n];
        out[(long)m * ldo + n] = v;
    }
}

// Tickets of the split hand-over: one zeroed uint32 per output tile, re-armed by the workgroup that takes the last one.  One array per
// STREAM: launches on a stream run in order, so the array is clean again before the next launch on it reads it, and launches on
// different streams (the engine runs weight gradients on two side streams) never share one.  Shared by the evenly scheduled NT kernel
// and the shares of the one-workgroup-per-tile kernel: both leave every ticket at zero.  (XV_TN_MAX_TILES per array: xv_gemm.h.)
unsigned* tn_tickets_for(hipStream_t s) {
    static std::mutex mu;
    static std::map<hipStream_t, unsigned*> pool;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find(s);
    if (it != pool.end()) return it->second;
    unsigned* t = nullptr;
    if (hipMalloc((void**)&t, XV_TN_MAX_TILES * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemset(t, 0, XV_TN_MAX_TILES * sizeof(unsigned)) != hipSuccess) return nullptr;      // (synchronous: visible to every stream)
    pool[s] = t;
    return t;
}

// "whole tiles + shares" (xv_launch_gemm_nt): shares per remaining tile, 0 = the schedule does not apply or does not pay.
// K-steps on the busiest CU = the whole tiles + ceil(rem * S / 256) shares of nk / S K-steps and ~10 K-steps of hand-over each; S is chosen
// so that the shares come out as (just under) a whole number per CU - 72 remaining tiles: 3 shares each = 216, at most one per CU, not 4 (288:
// two on some CUs) - and small on a tie (the tile's last share sums S slabs alone).  tests/test_streamk_schedule.py restates it.
int xv_nt_shares(int tiles, int ksteps, bool stats, bool beside_wgrad, size_t ws_bytes) {
    const int rem_tiles = tiles % 256, whole_per_cu = tiles / 256;
    if (rem_tiles < 1 || rem_tiles > 128) return 0;
    if (!(whole_per_cu >= 2 || (whole_per_cu == 1 && stats)) || (beside_wgrad && whole_per_cu == 3)) return 0;
    long best = 0;
    int best_s = 0;
    for (int sh = 2; sh <= 16 && ksteps / sh >= 6; ++sh) {
        const long t = (long)whole_per_cu * ksteps + (long)xv_cdiv((long)rem_tiles * sh, 256) * (ksteps / sh + 10) + sh;
        if (!best_s || t < best) { best = t; best_s = sh; }
    }
    const long t_dp = (long)xv_cdiv(tiles, 256) * ksteps;
    if (!best_s || best + best / 32 >= t_dp || (size_t)rem_tiles * best_s * BM * BN * sizeof(float) > ws_bytes) return 0;
    return best_s;
}

// Which schedule an NT launch runs (DESIGN.md section 4 "fp32 GEMM design" states the three and where each wins; the measurements behind every
// constant here are DESIGN.md Appendix A, rounds 3-4, and profiles/r04_nt_whole_plus_shares.txt / r04_ab_variants.txt):
//   DP      one workgroup per tile, dealt to the CUs by the hardware: cost ceil(tiles / 256) K-loops on the busiest CU
//   SK      one co-resident round of <= 768 persistent workgroups with equal runs of K-steps, tiles shared through slabs: total / 256 K-steps
//           + ~15 K-steps of hand-over per workgroup; its K loop is 4-8 % slower than DP's, so it only wins on tile-count quantisation
//   SHARES  DP for the first floor(tiles / 256) * 256 tiles, every remaining tile cut into `shares` K ranges behind them (xv_nt_shares)
//   SPLIT   few tiles and no BatchNorm statistics: split-K over the whole chip + a slab-sum launch (extraction one utterance at a time,
//           segment-level layers of batches > 128 chunks)
enum { XV_NT_DP = 0, XV_NT_SK = 1, XV_NT_SHARES = 2, XV_NT_SPLIT = 3 };
struct XvNtPlan { int kind, p_sk, shares, splits; bool shared_tiles; };      // shared_tiles (SK): some tile's K-steps are divided between workgroups
static XvNtPlan xv_nt_plan(int M, int N, int K, bool stats, bool co_running, bool have_ws, size_t ws_bytes, int forced /* XvEnv::nt_sched */) {
    const int tiles = xv_cdiv(M, BM) * xv_cdiv(N, BN), ksteps = xv_cdiv(K, BK);
    XvNtPlan pl = {XV_NT_DP, 1, 0, 1, false};
    const long total = (long)tiles * ksteps;
    const long p_sk = std::min<long>(std::min<long>(256L * XV_NT_SK_WPC, std::max<long>(1, total / 4)), 8L * tiles);
    const long t_sk = (total / p_sk) * xv_cdiv(p_sk, 256) + (15 * 16 / BK) * std::min<long>(XV_NT_SK_WPC, xv_cdiv(p_sk, 256));
    const long t_dp = tiles <= XV_RESIDENT_WGS ? (long)xv_cdiv(tiles, 256) * ksteps : total / 256 + ksteps / 2;
    bool sk = forced ? forced == 2 : t_sk + t_sk / 32 < t_dp;
    // Beside the weight-gradient stream (the data gradients) a launch with at least two whole tiles per CU is dealt one workgroup per tile: its
    // workgroups are never all resident at once there anyway (the other stream's kernel holds slots), so a partial last round is not the
    // cost `t_dp` prices, while the even schedule's slower K loop and hand-overs are.  [measured, round 6, same box, 6 alternated rounds,
    // profiles/r06_nt_co_running.txt] S1 (tdnn2's data gradient: 784 tiles, until now on the even schedule) -0.25 ... -0.4 %, S4 -0.4 %,
    // 64 x U{200..400} / S2 / S5 +-0.1 %; for every tile count -0.4 / -0.1 / +0.2 %, from three whole tiles per CU -0.3 / -0.3 / +0.1 %.
    if (!forced && co_running && tiles >= 512) sk = false;
    // ... and "whole tiles + shares" there only for long tiles (>= 100 K-steps): a share's hand-over (slab store, ticket, the last share sums the
    // others) is ~10 K-steps of latency whatever the tile's length, and beside the other stream's GEMM the partial round it avoids costs little.
    // [measured, round 6, same box, 4 alternated rounds, profiles/r06_nt_co_running.txt] S5 (ten layers of 32 / 96 K-step tiles at 128 x 400)
    // -1.0 %, every other shape within +-0.2 %; no shares at all beside the stream: S5 -1.2 %, 64 x U{200..400} +0.7 %, S2 +0.3 %.
    const int shares = forced || !have_ws || tiles > XV_TN_MAX_TILES || (co_running && ksteps < 100) ? 0 : xv_nt_shares(tiles, ksteps, stats, co_running, ws_bytes);
    if (shares) sk = false;
    const bool few = !stats && tiles < 192 && ksteps >= 8 && !forced;
    if (!few && sk) {
        const bool shared_tiles = total % p_sk != 0 || (total / p_sk) % ksteps != 0;
        if (!shared_tiles || ((size_t)p_sk * 2 * BM * BN * sizeof(float) <= ws_bytes && have_ws && tiles <= XV_TN_MAX_TILES)) {
            pl.kind = XV_NT_SK; pl.p_sk = (int)p_sk; pl.shared_tiles = shared_tiles;
            return pl;
        }
    }
    int splits = 1;
    if (!stats && tiles < XV_RESIDENT_WGS / 2 && ksteps >= 8) {
        splits = std::max(1, std::min(XV_RESIDENT_WGS / tiles, ksteps / 4));
        const long np = (long)xv_align(N, 4);
        // the slabs are written and read back: beyond ~8 MB the reduce costs more than the extra workgroups buy
        const long slab_cap = std::max<long>(8, (8L << 20) / ((long)M * np * (long)sizeof(float)));
        if (splits > slab_cap) splits = (int)slab_cap;
        while (splits > 1 && (size_t)splits * M * np * sizeof(float) > ws_bytes) --splits;
    }
    if (splits > 1) { pl.kind = XV_NT_SPLIT; pl.splits = splits; }
    else if (shares) { pl.kind = XV_NT_SHARES; pl.shares = shares; }
    return pl;
}
// diagnostics (tools/pmc_traffic.py maps S1's layers to the kernels that ran them with this): the schedule of an NT problem given ample workspace
extern "C" int xv_debug_nt_schedule(int M, int N, int K, int stats, int co_running) {
    const XvEnv* env = xv_env();
    return xv_nt_plan(M, N, K, stats != 0, co_running != 0, true, (size_t)1 << 32, env ? env->nt_sched : 0).kind;
}

// The <STATS, ROWS> instantiations of the two NT kernels, [stats][rows], and the one place that picks among them
static void (*const nt_kernels[2][2])(NTArgs) = {{xv_gemm_nt_kernel<false, false>, xv_gemm_nt_kernel<false, true>},
                                                 {xv_gemm_nt_kernel<true, false>, xv_gemm_nt_kernel<true, true>}};
static void (*const nt_sk_kernels[2][2])(NTSKArgs) = {{xv_gemm_nt_sk_kernel<false, false>, xv_gemm_nt_sk_kernel<false, true>},
                                                      {xv_gemm_nt_sk_kernel<true, false>, xv_gemm_nt_sk_kernel<true, true>}};
template <typename Args>
static void nt_launch(void (*const (&kernels)[2][2])(Args), bool stats, bool rows, dim3 grid, hipStream_t s, const Args& args) {
    hipLaunchKernelGGL(kernels[stats][rows], grid, dim3(256), 0, s, args);
}

int xv_launch_gemm_nt(hipStream_t s, const XvGemmNT& g) {
    XV_REQUIRE(g.K % 4 == 0 && g.lda % 4 == 0 && g.ldb % 4 == 0, "gemm_nt: K/lda/ldb must be multiples of 4 (K=%d lda=%ld ldb=%ld)", g.K, g.lda, g.ldb);
    XV_REQUIRE(((uintptr_t)g.A % 16) == 0 && ((uintptr_t)g.Bt % 16) == 0, "gemm_nt: operands must be 16-byte aligned");
    XV_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0 && g.a_rps > 0, "gemm_nt: empty problem");
    // xv_dma16 addresses every operand row as a 32-bit byte offset from the operand's base
    XV_REQUIRE(((long)xv_cdiv(g.M, g.a_rps) * g.a_pitch + 1) * g.lda * 4 < (1L << 32) && ((long)g.N + 1) * g.ldb * 4 < (1L << 32),
               "gemm_nt: an operand spans 4 GB or more (M=%d a_pitch=%d lda=%ld N=%d ldb=%ld): split the batch", g.M, g.a_pitch, g.lda, g.N, g.ldb);
    if (ensure_zero_page((size_t)g.K)) return 1;
    NTArgs p;
    p.zero = g_zero_page;
    p.stamp_half = xv_diag_half(g.M, g.N, g.K);
    p.A = g.A; p.lda = g.lda; p.a_rps = g.a_rps; p.a_pitch = g.a_pitch;
    p.Bt = g.Bt; p.ldb = g.ldb;
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.tiles_m = xv_cdiv(g.M, BM); p.tiles_n = xv_cdiv(g.N, BN);
    p.bias = g.bias; p.part_sum = nullptr; p.part_m2 = nullptr;
    p.n_whole = 0; p.shares = 0; p.slab = nullptr; p.tickets = nullptr;
#ifdef XV_NT_NO_ROWS      // (A/B build constant: the four-byte-store epilogue everywhere)
    p.row_store = 0;
#else
    p.row_store = (g.N % 4 == 0 && g.ldc % 4 == 0 && ((uintptr_t)g.C % 16) == 0) ? 1 : 0;
#endif
    const int tiles = p.tiles_m * p.tiles_n;
    const int ksteps = xv_cdiv(g.K, BK);
    const XvEnv* env = xv_env();
    if (!env) return 2;
    const XvNtPlan pl = xv_nt_plan(g.M, g.N, g.K, g.bn_part != nullptr, g.co_running != 0, g.ws != nullptr, g.ws_bytes, env->nt_sched);
    const int stats_kind = g.bn_part ? 0 : 1;      // XvProfScope kind
    if (pl.kind == XV_NT_SK) {
        NTSKArgs q;
        q.nk = ksteps;
        q.total = (long)tiles * ksteps;
        XV_REQUIRE(q.total < (1L << 31), "gemm_nt: %d tiles x %d K-steps exceed the evenly scheduled kernel's 32-bit unit index", tiles, ksteps);
        q.P = pl.p_sk;
        p.C = g.C; p.ldc = g.ldc; p.c_split_stride = 0; p.k_chunk = ksteps * BK;
        p.part_sum = g.bn_part; p.part_m2 = nullptr;
        q.g = p;
        q.slab = (float*)g.ws;
        q.tickets = pl.shared_tiles ? tn_tickets_for(s) : nullptr;
        XV_REQUIRE(!pl.shared_tiles || (q.tickets && ((uintptr_t)q.slab % 16) == 0), "gemm_nt: hand-over buffers unavailable");
        XvProfScope prof(s, stats_kind, 2.0 * g.M * g.N * g.K);
        nt_launch(nt_sk_kernels, g.bn_part != nullptr, p.row_store != 0, dim3(q.P), s, q);
        XV_LAUNCH_CHECK();
        return 0;
    }
    if (pl.kind != XV_NT_SPLIT) {      // one workgroup per tile, or whole tiles + shares of the remaining ones
        p.C = g.C; p.ldc = g.ldc; p.c_split_stride = 0; p.k_chunk = ksteps * BK;
        dim3 grid(tiles, 1, 1);
        if (pl.kind == XV_NT_SHARES) {
            p.n_whole = tiles / 256 * 256;
            p.shares = pl.shares;
            p.slab = (float*)g.ws;
            p.tickets = tn_tickets_for(s);
            XV_REQUIRE(p.tickets && ((uintptr_t)p.slab % 16) == 0, "gemm_nt: hand-over buffers unavailable");
            grid.x = p.n_whole + (tiles - p.n_whole) * pl.shares;
        }
        XvProfScope prof(s, stats_kind, 2.0 * g.M * g.N * g.K);
        p.part_sum = g.bn_part;      // (null without statistics; part_m2 is null in every launch)
        nt_launch(nt_kernels, g.bn_part != nullptr, p.row_store != 0, grid, s, p);
        XV_LAUNCH_CHECK();
        return 0;
    }
    // split-K over the whole chip + a slab-sum launch (few tiles, no BatchNorm statistics to emit)
    int splits = pl.splits;
    const long np = (long)xv_align(g.N, 4);
    XV_REQUIRE((size_t)splits * g.M * np * sizeof(float) <= g.ws_bytes, "gemm_nt: workspace too small (%zu bytes)", g.ws_bytes);
    p.C = (float*)g.ws; p.ldc = np; p.c_split_stride = (long)g.M * np;
#ifndef XV_NT_NO_ROWS
    p.row_store = g.N % 4 == 0 ? 1 : 0;      // (the slab is 256-byte aligned, np and M * np are multiples of 4)
#endif
    p.k_chunk = xv_cdiv(ksteps, splits) * BK;
    splits = xv_cdiv(g.K, p.k_chunk);
    p.bias = nullptr;
    dim3 grid(tiles, 1, splits);
    {
        XvProfScope prof(s, 1, 2.0 * g.M * g.N * g.K);
        nt_launch(nt_kernels, false, p.row_store != 0, grid, s, p);
    }
    XV_LAUNCH_CHECK();
    long total = (long)g.M * g.N;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(xv_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, s, (const float*)g.ws, splits,
                       (long)g.M * np, g.M, g.N, (int)np, g.bias, g.C, g.ldc);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_affine_forward(void* stream, const float* x, int segs, int t_in, int c_pad, int k, const float* wt,
                                 const float* bias, float* z, int o, int ldz, float* bn_part, void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_in >= k && c_pad > 0 && o > 0 && ldz >= o, "affine_forward: bad shape (t_in=%d k=%d)", t_in, k);
    XvGemmNT g = {};
    g.A = x; g.lda = c_pad; g.a_rps = t_in - k + 1; g.a_pitch = t_in;
    g.Bt = wt; g.ldb = (long)k * c_pad;
    g.C = z; g.ldc = ldz;
    g.M = segs * (t_in - k + 1); g.N = o; g.K = k * c_pad;
    g.bias = bias; g.bn_part = bn_part; g.ws = ws; g.ws_bytes = ws_bytes;
    return xv_launch_gemm_nt((hipStream_t)stream, g);
}

int xv_affine_dgrad_ld(hipStream_t stream, const float* dz_pad, int ldo, int segs, int t_out, int o, int k, const float* wf, float* dx, int c,
                       void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && k >= 1 && t_out >= 1 && o > 0 && c > 0 && ldo >= o && (ldo == o || k == 1), "affine_dgrad: bad shape (a row pitch needs k = 1)");
    XvGemmNT g = {};
    g.A = dz_pad; g.lda = ldo; g.a_rps = t_out + k - 1; g.a_pitch = t_out + 2 * (k - 1);
    g.Bt = wf; g.ldb = (long)k * o;
    g.C = dx; g.ldc = c;
    g.M = segs * (t_out + k - 1); g.N = c; g.K = k * o;
    g.ws = ws; g.ws_bytes = ws_bytes;
    g.co_running = 1;          // the data gradient runs beside the layer's weight gradient (xv_engine_bwd.hip: two streams)
    return xv_launch_gemm_nt(stream, g);
}
extern "C" int xv_affine_dgrad(void* stream, const float* dz_pad, int segs, int t_out, int o, int k, const float* wf, float* dx,
                               int c, void* ws, size_t ws_bytes) {
    return xv_affine_dgrad_ld((hipStream_t)stream, dz_pad, o, segs, t_out, o, k, wf, dx, c, ws, ws_bytes);
}
