// Device pieces shared by the fp32 GEMM kernels (xv_gemm_nt.hip, xv_gemm_tn.hip; xcd_swizzle also by xv_gemm16_nt.hip / xv_gemm16_tn.hip), each stated once: the LDS
// image of the NT kernels, the XCD swizzle, the hardware lane / wave helpers and the two tile epilogues of the NT kernels.  Plain
// __forceinline__ functions: every kernel keeps the instruction sequence it had (profiles/gemm_split_isa.txt).
// What is NOT here, although both NT kernels spell it the same way: zeroing the 2 x 2 accumulators, the fragment reads and MFMAs of one
// K-step, and the slab publish / slab accumulate of a shared tile.  Each was tried as a function taking references; hipcc then orders the
// instructions of at least one kernel differently (same registers, another stream: the table in profiles/gemm_split_isa.txt), so those
// sites stay written out and say so.
#pragma once
#include "xv_common.h"
#include "xv_gemm.h"
#include "xv_handoff.h"

// NT LDS image: [128 rows][XV_TILE_K floats], no padding, 16-byte chunk c of row r stored at chunk
// c ^ f(r) with f(r) = (r >> NT_SW_SHIFT) & (NT_KQ-1).  ds_read_b128 (banks = 16 slots of 16 B,
// 16-lane groups reading 16 different rows at one chunk index) sees 16 distinct slots, and
// ds_write_b128 (8-lane groups = 2 rows x 4 chunks at BK=16) sees 8 distinct slots: the padded
// image of the first build had 2-way write conflicts at BK=16 (SQ_LDS_BANK_CONFLICT, profiles/).
#define NT_PITCH XV_TILE_K
#define NT_SW_SHIFT (XV_TILE_K == 16 ? 2 : 1)
#define NT_SWZ(row) ((((row) >> NT_SW_SHIFT) & (XV_TILE_K / 4 - 1)))
static_assert(XV_TILE_K == 16 || XV_TILE_K == 32, "K-step must be 16 or 32");
#define NT_KQ (XV_TILE_K / 4)               // float4 per tile row
#define NT_RPT (XV_TILE_M * NT_KQ / 256)    // tile rows staged per thread (2 or 4)

__device__ __forceinline__ int xcd_swizzle(int bid, int nwg) {
    // blocks b and b+8 share an XCD (round-robin dispatch): hand each XCD a contiguous run of
    // tiles so the n-tiles of one m-tile (same A rows) and neighbouring m-tiles (overlapping
    // context windows) hit the same L2.  Bijective for any nwg.
    int xcd = bid & 7, idx = bid >> 3, q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Epilogue of the NT kernels: acc += bias, C tile <- acc.  The bias is added in a pass of its own in front of the stores:
// written as "v = acc + bias; if (in range) C = v" per element, hipcc put the bias load's s_waitcnt vmcnt(0) inside every
// predicated store block - and stores count on vmcnt too, so each of the 64 stores of a lane waited for the previous one to
// retire (a serialised ~30k-cycle tail per tile, with every workgroup of a one-round grid in it at the same time).  Interior
// tiles store without predication.
__device__ __forceinline__ void nt_store_tile(f32x16 (&acc)[2][2], float* __restrict__ C, long ldc, const float* __restrict__ bias,
                                              int m0, int n0, int M, int N, int wr, int wc, int li, int lh) {
    asm volatile("" : "+v"(wr), "+v"(wc), "+v"(li), "+v"(lh));      // (opaque copies: see nt_store_tile_rows)
    if (bias) {
        float bias_v[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = n0 + wc * 64 + b * 32 + li;
            bias_v[b] = bias[min(n, N - 1)];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] += bias_v[b];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) asm volatile("" : "+v"(acc[a][b]));      // keeps hipcc from sinking the adds back into the store blocks
    }
    float* c0 = C + (long)(m0 + wr * 64 + 4 * lh) * ldc + n0 + wc * 64 + li;
    if (m0 + XV_TILE_M <= M && n0 + XV_TILE_N <= N) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) c0[(long)(a * 32 + (r & 3) + 8 * (r >> 2)) * ldc + b * 32] = acc[a][b][r];
    } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int n = n0 + wc * 64 + b * 32 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wr * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (m < M && n < N) c0[(long)(a * 32 + (r & 3) + 8 * (r >> 2)) * ldc + b * 32] = acc[a][b][r];
                }
            }
    }
}

// The same epilogue through the (idle) staging LDS: the accumulators of one 32-row block per wave - 64 rows x 128 columns of the tile, exactly
// the 32 KB of the two stages - are written as they stand (one column per lane: 128 consecutive bytes per half wave, no bank conflict), the
// workgroup meets, and every thread reads whole-row float4 and stores 16 bytes: a half wave stores one 512-byte row segment per instruction,
// 16 store instructions per lane and tile instead of 64 four-byte ones (whose latency chain was the 10 us epilogue of a 32-K-step tile,
// exposed whenever the workgroups of a launch end together: every one-round launch).  Two passes (a = 0, 1).  Needs C and ldc 16-byte aligned
// and N a multiple of 4; the caller falls back to nt_store_tile otherwise.  Ends behind a barrier (the LDS may be reused at once).
__device__ __forceinline__ void nt_store_tile_rows(f32x16 (&acc)[2][2], float* smem, float* __restrict__ C, long ldc, const float* __restrict__ bias,
                                                   int m0, int n0, int M, int N, int tid, int wr, int wc, int li, int lh) {
    // (opaque copies: in the evenly scheduled kernel this runs inside the loop over a workgroup's tiles, and hipcc otherwise hoists the lane
    // constants below out of it - live across the K loop, they were what that kernel spilled)
    asm volatile("" : "+v"(tid), "+v"(wr), "+v"(wc), "+v"(li), "+v"(lh));
    if (bias) {
        float bias_v[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) bias_v[b] = bias[min(n0 + wc * 64 + b * 32 + li, N - 1)];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] += bias_v[b];
    }
    // image [64 rows: wr * 32 + row of the 32-row block][128 columns]
    float* wbase = smem + (wr * 32 + 4 * lh) * XV_TILE_N + wc * 64 + li;
    const int rq = tid >> 5, cq = (tid & 31) * 4;                // reader: rows rq, rq + 8, ... of the image, columns cq .. cq + 3
    const bool col_ok = n0 + cq < N;                              // (N % 4 == 0: all four or none)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) wbase[((r & 3) + 8 * (r >> 2)) * XV_TILE_N + b * 32] = acc[a][b][r];
        __syncthreads();
        f32x4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *(const f32x4*)(smem + (rq + 8 * i) * XV_TILE_N + cq);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = rq + 8 * i;                             // image row: wr' = q / 32, row of the block = q % 32
            const int m = m0 + (q >> 5) * 64 + a * 32 + (q & 31);
            if (m < M && col_ok) *(f32x4*)(C + (long)m * ldc + n0 + cq) = v[i];
        }
        __syncthreads();
    }
}

// The evenly scheduled kernel rotates the issue priority of its waves every K-step - priority = (K-step + the wave's slot in its SIMD) mod 4 -
// so that the co-resident workgroups take turns at the top and finish together; NOT in the one-workgroup-per-tile kernel, whose multi-round
// launches want their oldest workgroups to finish first (note 1).
// the lane's index from the hardware (two vector instructions) instead of from threadIdx.x: code behind the K loop of the evenly scheduled kernel
// rebuilds its thread coordinates from this and the (scalar) wave index, so nothing derived from threadIdx.x stays live - spilled - across the loop
__device__ __forceinline__ int xv_lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int xv_wave_slot() { return __builtin_amdgcn_s_getreg(4 | (3 << 11)) & 15; }      // HW_ID.WAVE_ID: differs between the waves of one SIMD
__device__ __forceinline__ void xv_rot_prio(int x) {
    switch (x & 3) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}
