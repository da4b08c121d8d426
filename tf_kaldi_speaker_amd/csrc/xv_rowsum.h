// The row sum of the one-wave-per-row kernels of scoring (xv_score.hip) and of the back end (xv_backend.hip), and the operand checks their
// launchers share.  gfx950 only.
#pragma once
#include "xv_common.h"
#include "xv_ew.h"

#define SC_ROWS_PER_WG 4          // one wave per row / trial, four to a workgroup of 256

// Σ over one row by one wave.  The add chain the row kernels share: a lane's partial takes the elements (vector form: float4 groups)
// lane, lane + 64, ... one fma each - ceil(d / 64) fmas in the scalar form, 4 * ceil(d / 256) in the vector form - and the butterfly
// adds six more, so no sum is longer than
//     chain(d) = 4 * ceil(d / 256) + 6
// roundings (the scalar form's ceil(d / 64) + 6 never exceeds it).  tests/test_gpu_score.py derives its tolerance from this figure.
// WGT (the PLDA normalisation): b holds psi and the term is u * (u / (psi[c] + inv_n)) - the same lanes, the same chain.
template <bool VEC, bool SUB, bool WGT = false>
__device__ __forceinline__ float sc_row_dot(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean, int d, int lane,
                                            float inv_n = 0.f) {
    float acc = 0.f;
    if (VEC) {
        for (int q = lane; q < d / 4; q += XV_WAVE) {
            f32x4 u = *(const f32x4*)(a + 4 * q), v = *(const f32x4*)(b + 4 * q);
            if (SUB) {      // (the prepare kernel: a == b, the row minus the mean dotted with itself)
                const f32x4 m = *(const f32x4*)(mean + 4 * q);
                u -= m;
                v = u;
            }
            if (WGT) v = u / (v + inv_n);
            acc = fmaf(u.x, v.x, acc); acc = fmaf(u.y, v.y, acc); acc = fmaf(u.z, v.z, acc); acc = fmaf(u.w, v.w, acc);
        }
    } else {
        for (int c = lane; c < d; c += XV_WAVE) {
            float u = a[c], v = b[c];
            if (SUB) { u -= mean[c]; v = u; }
            if (WGT) v = u / (v + inv_n);
            acc = fmaf(u, v, acc);
        }
    }
    return wave_sum(acc);
}

static inline bool sc_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
// [a, a + an) and [b, b + bn) floats share an address
static inline bool sc_overlap(const float* a, size_t an, const float* b, size_t bn) {
    return (uintptr_t)a < (uintptr_t)(b + bn) && (uintptr_t)b < (uintptr_t)(a + an);
}
