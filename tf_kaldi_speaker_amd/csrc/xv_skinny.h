#pragma once
#include "xv_common.h"

// Segment-level GEMM C[M][N] = A[M][K] . Bt[N][K]^T, M <= 128 rows (the chunks of one batch), with the split-K sum and the consumer's
// per-column work in the same launch (xv_skinny.hip).  `ws` holds the [splits][N/32][128][32] slabs, `tickets` one zeroed uint32 per
// 32 columns (left zeroed).  Optional row term before the epilogue: acc[m][n] += (row_norm[m] > 0 ? row_coef[m] / row_norm[m] : 0) * X[m][n].
enum { XV_SK_PLAIN = 0,      // C = acc + bias
       XV_SK_BN_FWD = 1,     // C = z = acc + bias; training-mode BatchNorm over the M rows (+ activation) -> a_out; vectors and moving averages written
       XV_SK_BN_BWD = 2 };   // acc = d a of a BatchNorm(+activation) layer with pre-BN tensor z: C = dz, dgamma / dbeta / dbias / dalpha written
struct XvSkinny {
    const float* A; long lda;
    const float* Bt; long ldb;
    int M, N, K;
    float* C; long ldc;                      // also the leading dimension of z and a_out
    const float* bias;
    const float* row_coef; const float* row_norm; const float* X; long ldx;
    int epi;
    const float* gamma; const float* beta; float eps, momentum; int unbiased; float* mmean; float* mvar;
    float* mean; float* invstd; float* scale; float* shift;      // written by BN_FWD, read by BN_BWD
    int relu; const float* slope; float* a_out;
    const float* z; float* dgamma; float* dbeta; float* dbias; float* dalpha;
    void* ws; size_t ws_bytes; uint32_t* tickets;
};
int xv_launch_skinny(hipStream_t s, const XvSkinny& g);
size_t xv_skinny_tickets(int max_n);
