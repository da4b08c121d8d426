// Internal interface of the GEMM units (xv_gemm_nt.hip, xv_gemm_tn.hip, xv_gemm16_nt.hip, xv_gemm16_tn.hip): tile geometry, the zero page, the ticket pool, the
// launch structs and launchers, the split functions the callers size workspaces with, and live launch timing.
#pragma once
#include "xv_common.h"

// ---- GEMM geometry shared between launchers and the engine -------------------------
#define XV_TILE_M 128
#define XV_TILE_N 128
#ifndef XV_TILE_K
#define XV_TILE_K 16
#endif
// workgroups of 256 threads that are resident per CU (== waves per SIMD); LDS and VGPR budgets of
// both GEMM kernels are sized for it, and the split policies aim at one co-resident round.
#ifndef XV_WGS_PER_CU
#define XV_WGS_PER_CU (XV_TILE_K == 16 ? 4 : 2)
#endif
#define XV_RESIDENT_WGS (256 * XV_WGS_PER_CU)

// A device page of at least `floats` (and XV_ZERO_PAGE_FLOATS) zeros (xv_gemm_nt.hip): out-of-range rows / k of a GEMM operand are redirected
// to it (the select is on the address, loads stay unconditional); "base + k" stays inside the page for every k < K <= floats
#define XV_ZERO_PAGE_FLOATS 16384
const float* xv_zero_page(size_t floats = XV_ZERO_PAGE_FLOATS);

// Tickets of the split hand-over (xv_gemm_nt.hip): XV_TN_MAX_TILES zeroed uint32 per STREAM, one per output tile, re-armed by the workgroup that
// takes the last one; null when the allocation fails
#define XV_TN_MAX_TILES 16384
unsigned* tn_tickets_for(hipStream_t s);

// Internal GEMM launchers (xv_gemm_nt.hip, xv_gemm_tn.hip).
// C[m][n] (+)= sum_k A[rowmap(m)][k] * Bt[n][k]   ("NT", both operands k-contiguous)
// rowmap(m) = (m / a_rps) * a_pitch + (m % a_rps) rows of lda floats.
struct XvGemmNT {
    const float* A; long lda; int a_rps; int a_pitch;
    const float* Bt; long ldb;
    float* C; long ldc;
    int M, N, K;
    const float* bias;      // optional, [N]
    float* bn_part;         // optional, [4][tiles_m][N]: sum, centred squares, min, max (xv_epilogue.h)
    void* ws; size_t ws_bytes;
    int co_running;         // 1: another GEMM shares the chip (the backward pass: data gradient beside weight gradient) - see xv_launch_gemm_nt
};
int xv_launch_gemm_nt(hipStream_t s, const XvGemmNT& g);
// xv_affine_dgrad / xv_affine_wgrad (include/xvector_hip.h) for a dz whose rows are ldo >= o floats apart (the pooled layer's, on the 128-byte grid)
int xv_affine_dgrad_ld(hipStream_t stream, const float* dz_pad, int ldo, int segs, int t_out, int o, int k, const float* wf, float* dx, int c,
                       void* ws, size_t ws_bytes);
int xv_affine_wgrad_ld(hipStream_t stream, const float* x, int segs, int t_in, int c_pad, int k, int c, const float* dz, int ldo, int dz_seg_pitch,
                       int dz_row0, int o, const float* kernel, float l2_scale, float* dkernel, void* ws, size_t ws_bytes);

// P[z][m][n] = sum_{r in chunk z} A[amap(r)][m] * B[bmap(r)][n]   ("TN", reduction over rows)
struct XvGemmTN {
    const float* A; long lda; int a_rps; int a_pitch;   // [R] rows mapped, M columns used
    const float* B; long ldb; int b_rps; int b_pitch;   // [R] rows mapped, N columns used
    int M, N, R;
    float* P;            // slabs [splits][M][N]
    int splits;          // chosen by xv_tn_splits (xv_tn_splits_direct when `direct`)
    int direct;          // 1: the caller stores an unsplit result straight into its destination (P = the [M][N] result when splits == 1): a short
                         // reduction over many tiles is then not split at all (the loss head's weight gradient)
};
int xv_tn_splits(int M, int N, int R);
int xv_tn_splits_direct(int M, int N, int R);
int xv_nt_shares(int tiles, int ksteps, bool stats, bool beside_wgrad, size_t ws_bytes);      // NT: shares per remaining tile of the "whole tiles + shares" schedule (0: not used)
int xv_launch_gemm_tn(hipStream_t s, const XvGemmTN& g);
// out[(j*C + c)][n] = sum_z P[z][j*c_pad + c][n] (+ l2 * w[(j*C + c)][n]): the slab sum behind a weight-gradient GEMM (xv_gemm_tn.hip)
int xv_launch_wgrad_reduce(hipStream_t s, const float* P, int splits, int k, int C, int c_pad, int n_in, int n_out, const float* w,
                           long ldw, float l2, float* out, long ldo);

// ---- split-precision (f16x3) GEMMs on fp16 planes (xv_gemm16_nt.hip, xv_gemm16_tn.hip; xv_gemm16.h) ---
struct XvGemm16NT {
    const void* A; long lda; long a_plane; int a_rps; int a_pitch;   // planes [2][rows][lda] fp16
    const void* Bt; long ldb; long b_plane;
    float* C; long ldc;
    int M, N, K;
    const float* bias;
    float* bn_part;                       // optional [4][tiles_m][N]
    const unsigned* a_amax; const unsigned* b_amax;   // device: float bits of the operands' max |x| (scale source)
    // optional data-gradient epilogue (xv_epilogue.h XvBwdStats): C is d a of a BN+ReLU layer whose pre-BN tensor is bwd_z [M][N]
    const float* bwd_z; const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; const float* bwd_invstd;
    float* bwd_part;                      // [tiles_m][3][N]
};
int xv_launch_gemm16_nt(hipStream_t s, const XvGemm16NT& g);
struct XvGemm16TN {
    const void* A; long lda; long a_plane; int a_pitch;
    const void* B; long ldb; long b_plane; int b_pitch;
    int rps;
    int M, N, R;
    float* P; int splits;                 // slabs [splits][M][N]; splits from xv_tn16_splits
    const unsigned* a_amax; const unsigned* b_amax;
};
int xv_tn16_splits(int M, int N, int R);
int xv_launch_gemm16_tn(hipStream_t s, const XvGemm16TN& g);

// Live launch timing (xv_profile_begin/end, xv_runtime.hip): brackets one GEMM launch with hipEvents on its stream.
struct XvProfScope {
    hipStream_t s; int idx;
    XvProfScope(hipStream_t st, int kind, double flops);
    ~XvProfScope();
};
