// The row sum and the row-wise store of the one-wave-per-row kernels of scoring (xv_score.hip) and of the back end (xv_backend.hip,
// xv_backend_cohort.hip): the lanes are walked here, a kernel states its term.  (Their launch side: xv_score_launch.h.)  gfx950 only.
#pragma once
#include "xv_common.h"
#include "xv_ew.h"

#define SC_ROWS_PER_WG 4          // one wave per row / trial, four to a workgroup of 256

// a float4 group's four columns in order: acc = term(acc, v0[k], v1[k], ...) for k = x, y, z, w
template <class Term, class... V>
__device__ __forceinline__ float sc_term4(float acc, Term term, V... v) {
    acc = term(acc, v.x...); acc = term(acc, v.y...); acc = term(acc, v.z...); acc = term(acc, v.w...);
    return acc;
}

// Σ over one row by one wave: acc = term(acc, row0[c], row1[c], ...) once per column c < d, then the butterfly.  The add chain the row
// kernels share: a lane's partial takes the columns (vector form: float4 groups, the four components in order) lane, lane + 64, ... one
// term each - ceil(d / 64) terms in the scalar form, 4 * ceil(d / 256) in the vector form - and the butterfly adds six more, so with a
// term of one fma on acc no sum is longer than
//     chain(d) = 4 * ceil(d / 256) + 6
// roundings (the scalar form's ceil(d / 64) + 6 never exceeds it); a term of two fmas on acc (backend_plda_trials_kernel) doubles the lane's
// part only.  tests/test_gpu_score.py derives its tolerance from this figure.
template <bool VEC, class Term, class... Row>
__device__ __forceinline__ float sc_row_sum(int d, int lane, Term term, const Row*... row) {
    float acc = 0.f;
    if (VEC) {
        for (int q = lane; q < d / 4; q += XV_WAVE) acc = sc_term4(acc, term, *(const f32x4*)(row + 4 * q)...);
    } else {
        for (int c = lane; c < d; c += XV_WAVE) acc = term(acc, row[c]...);
    }
    return wave_sum(acc);
}

// y[c] = f(row0[c], row1[c], ...) for c < d, 0 for d <= c < ldy, by the lanes of sc_row_sum: in place (y == row0) a lane reads back exactly
// the elements it then overwrites, and the padding belongs to the row.  f is element-wise and takes floats or float4 groups alike.
template <bool VEC, class F, class... Row>
__device__ __forceinline__ void sc_row_store(float* y, long ldy, int d, int lane, F f, const Row*... row) {
    if (VEC) {
        for (int q = lane; q < (int)(ldy / 4); q += XV_WAVE) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < d / 4) v = f(*(const f32x4*)(row + 4 * q)...);
            *(f32x4*)(y + 4 * q) = v;
        }
    } else {
        for (int c = lane; c < (int)ldy; c += XV_WAVE) y[c] = c < d ? f(row[c]...) : 0.f;
    }
}
