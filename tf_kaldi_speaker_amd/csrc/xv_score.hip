// Cosine trial scoring with adaptive symmetric score normalisation (AS-norm): what ivector-subtract-global-mean | ivector-normalize-length,
// ivector-compute-dot-products and the cohort statistics of an AS-norm back end do behind the reference's extract.py, on embedding
// matrices that live on the device.  Four ops: rows centred and scaled to unit length (score_prepare), trial dot products with the
// optional normalisation (score_trials), that normalisation alone on scores already on the device (score_normalize), and per row the
// mean / deviation of its top-k cohort scores (score_cohort_stats: the project's fp32 NT GEMM into a score slab, then an exact radix
// select per row, xv_select.h).  No floating-point atomics and no cross-workgroup hand-over in
// these kernels (the select's histogram is integer LDS atomics: a count does not depend on the order of its increments): a result
// depends on the shape of the call only, so it is the same bits every time.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_rowsum.h"            // sc_row_sum and chain(d), sc_row_store, SC_ROWS_PER_WG
#include "xv_score_launch.h"      // the operand checks, sc_launch_rows, sc_gemm_nt, sc_tile_rows
#include "xv_select.h"            // sc_select_kernel: the exact top-k selection and its statistics; SC_TILE_ROWS, sc_slab_pitch

// y[r][c] = v * rsqrt(max(Σ v², 1e-12)), v = x[r][c] - mean[c], for c < d; y[r][d .. ldy) = 0.  One wave per row.  In place (y == x,
// ldy == ldx) a lane reads back exactly the elements it then overwrites, and the padding belongs to the row (sc_row_store).
template <bool VEC, bool SUB>
__global__ __launch_bounds__(256) void score_prepare_kernel(const float* x, int rows, int d, long ldx, const float* __restrict__ mean, float* y, long ldy) {
    XV_EW_PRIORITY();
    const int r = blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* xr = x + (long)r * ldx;
    float* yr = y + (long)r * ldy;
    const float ss = SUB ? sc_row_sum<VEC>(d, lane, [](float acc, float u, float m) { u -= m; return fmaf(u, u, acc); }, xr, mean)
                         : sc_row_sum<VEC>(d, lane, [](float acc, float u, float v) { return fmaf(u, v, acc); }, xr, xr);
    const float inv = rsqrtf(fmaxf(ss, 1e-12f));
    if (SUB) sc_row_store<VEC>(yr, ldy, d, lane, [inv](auto v, auto m) { v -= m; return v * inv; }, xr, mean);
    else sc_row_store<VEC>(yr, ldy, d, lane, [inv](auto v) { return v * inv; }, xr);
}

// AS-norm of a score s with the cohort statistics (μ, σ) of its enrolment row a and its test row b: one expression, so score_trials_kernel
// and score_normalize_kernel give the same bits for the same s
__device__ __forceinline__ float sc_as_norm(float s, const float* __restrict__ e_stats, int a, const float* __restrict__ t_stats, int b) {
    return 0.5f * ((s - e_stats[2 * (long)a]) / e_stats[2 * (long)a + 1] + (s - t_stats[2 * (long)b]) / t_stats[2 * (long)b + 1]);
}

// out[j] = s = Σ_c e[ei[j]][c] * t[ti[j]][c], or with the row statistics 0.5 * ((s - μe) / σe + (s - μt) / σt).  One wave per trial;
// the sum is sc_row_sum's (chain(d) of xv_rowsum.h).
template <bool VEC>
__global__ __launch_bounds__(256) void score_trials_kernel(const float* __restrict__ e, long lde, const float* __restrict__ t, long ldt, int d,
                                                           const int* __restrict__ ei, const int* __restrict__ ti, long m,
                                                           const float* __restrict__ e_stats, const float* __restrict__ t_stats,
                                                           float* __restrict__ out) {
    XV_EW_PRIORITY();
    const long j = (long)blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= m) return;
    const int a = ei[j], b = ti[j];
    float s = sc_row_sum<VEC>(d, lane, [](float acc, float u, float v) { return fmaf(u, v, acc); }, e + (long)a * lde, t + (long)b * ldt);
    if (e_stats) s = sc_as_norm(s, e_stats, a, t_stats, b);
    if (lane == 0) out[j] = s;
}

// (score_cohort_stats selects with sc_select_kernel<ScSlabRow> of xv_select.h: the plain slab element)

// out[j] = sc_as_norm of scores[j] with the statistics of rows ei[j] / ti[j]: the normalisation of score_trials_kernel on scores that are
// on the device already (the PLDA log-likelihood ratios).  One thread per trial; out == scores is in place.
__global__ __launch_bounds__(256) void score_normalize_kernel(const float* scores, const int* __restrict__ ei, const int* __restrict__ ti, long m,
                                                              const float* __restrict__ e_stats, const float* __restrict__ t_stats, float* out) {
    XV_EW_PRIORITY();
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    out[j] = sc_as_norm(scores[j], e_stats, ei[j], t_stats, ti[j]);
}

extern "C" int xv_score_prepare(void* stream, const float* x, int rows, int d, int ldx, const float* mean, float* y, int ldy) {
    XV_REQUIRE(x && y && rows > 0 && d > 0, "score_prepare: bad arguments");
    XV_REQUIRE(ldx >= d && ldy >= d, "score_prepare: a pitch is below d (d=%d ldx=%d ldy=%d)", d, ldx, ldy);
    if (const int rc = sc_check_row_out("score_prepare", "x", x, ldx, "y", y, ldy, rows, d, "mean", mean)) return rc;
    return sc_launch_rows(mean ? score_prepare_kernel<true, true> : score_prepare_kernel<true, false>,
                          mean ? score_prepare_kernel<false, true> : score_prepare_kernel<false, false>,
                          sc_vec_ok(d, {ldx, ldy}, {x, y, mean}), rows, nullptr, (hipStream_t)stream, x, rows, d, ldx, mean, y, ldy);
}

extern "C" int xv_score_trials(void* stream, const float* e, int lde, int ne, const float* t, int ldt, int nt, int d, const int32_t* ei,
                               const int32_t* ti, int64_t m, const float* e_stats, const float* t_stats, float* out) {
    XV_REQUIRE(e && t && ei && ti && out && ne > 0 && nt > 0 && d > 0 && m > 0, "score_trials: bad arguments");
    XV_REQUIRE(lde >= d && ldt >= d, "score_trials: a pitch is below d (d=%d lde=%d ldt=%d)", d, lde, ldt);
    XV_REQUIRE((e_stats != nullptr) == (t_stats != nullptr), "score_trials: e_stats and t_stats must both be given or both be NULL");
    return sc_launch_rows(score_trials_kernel<true>, score_trials_kernel<false>, sc_vec_ok(d, {lde, ldt}, {e, t}), m,
                          "score_trials: too many trials in one call (%lld)", (hipStream_t)stream, e, lde, t, ldt, d, ei, ti, m, e_stats, t_stats, out);
}

extern "C" size_t xv_score_cohort_workspace_bytes(int rows, int n_cohort, int d) {
    (void)d;
    return xv_align((size_t)(rows > 0 ? rows : 1), SC_TILE_ROWS) * sc_slab_pitch(n_cohort) * sizeof(float);
}

extern "C" int xv_score_cohort_stats(void* stream, const float* x, int ldx, int rows, const float* cohort, int ldc, int n_cohort, int d,
                                     int top_k, float* stats, void* ws, size_t ws_bytes) {
    XV_REQUIRE(top_k > 0, "score_cohort_stats: top_k must be positive (got %d)", top_k);
    XV_REQUIRE(n_cohort > 0, "score_cohort_stats: n_cohort must be positive (got %d)", n_cohort);
    XV_REQUIRE(x && cohort && stats && rows > 0 && d > 0, "score_cohort_stats: bad arguments");
    const int kd = (int)xv_align(d, 4);      // the GEMM's K: columns d .. kd of both operands are read (score_prepare wrote them as zero)
    XV_REQUIRE(ldx >= kd && ldc >= kd, "score_cohort_stats: both pitches must reach d rounded up to 4 (d=%d ldx=%d ldc=%d)", d, ldx, ldc);
    const size_t pitch = sc_slab_pitch(n_cohort);
    XV_REQUIRE(ws && sc_aligned16(ws) && ws_bytes / (pitch * sizeof(float)) >= SC_TILE_ROWS,
               "score_cohort_stats: workspace of %zu bytes, at least one %d-row tile of %zu needed (16-byte aligned)", ws_bytes, SC_TILE_ROWS,
               (size_t)SC_TILE_ROWS * pitch * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    const int tile = sc_tile_rows(ws_bytes / (pitch * sizeof(float)), ldx);
    const int k = top_k < n_cohort ? top_k : n_cohort;
    for (int r0 = 0; r0 < rows; r0 += tile) {
        const int m = rows - r0 < tile ? rows - r0 : tile;
        if (const int rc = sc_gemm_nt(s, x + (size_t)r0 * ldx, ldx, cohort, ldc, (float*)ws, (long)pitch, m, n_cohort, kd)) return rc;
        hipLaunchKernelGGL(sc_select_kernel<ScSlabRow>, dim3(m), dim3(SC_SEL_THREADS), 0, s, (const float*)ws, (long)pitch, n_cohort, k, stats + 2 * (size_t)r0);
        XV_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int xv_score_dense(void* stream, const float* x, int ldx, int n, int d, float* out, int ldo) {
    XV_REQUIRE(x && out && n > 0 && d > 0, "score_dense: bad arguments");
    const int kd = (int)xv_align(d, 4);      // the GEMM's K: columns d .. kd of the rows are read (score_prepare wrote them as zero)
    XV_REQUIRE(ldx >= kd, "score_dense: the pitch must reach d rounded up to 4 (d=%d ldx=%d)", d, ldx);
    XV_REQUIRE(ldo >= n, "score_dense: the pitch of out is below n (n=%d ldo=%d)", n, ldo);
    XV_REQUIRE(!sc_overlap(x, (size_t)(n - 1) * ldx + kd, out, (size_t)(n - 1) * ldo + n), "score_dense: x and out overlap");
    return sc_gemm_nt((hipStream_t)stream, x, ldx, x, ldx, out, ldo, n, n, kd);      // xv_score_cohort_stats's GEMM with the rows as their own cohort
}

extern "C" int xv_score_normalize(void* stream, const float* scores, const int32_t* ei, const int32_t* ti, int64_t m, const float* e_stats,
                                  const float* t_stats, float* out) {
    XV_REQUIRE(scores && ei && ti && e_stats && t_stats && out && m > 0, "score_normalize: bad arguments");
    XV_REQUIRE(m <= (int64_t)256 * 0x7fffffff, "score_normalize: too many trials in one call (%lld)", (long long)m);
    XV_REQUIRE(out == scores || !sc_overlap(scores, (size_t)m, out, (size_t)m), "score_normalize: scores and out overlap (in place needs out == scores)");
    hipLaunchKernelGGL(score_normalize_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, (const int*)ei, (const int*)ti,
                       (long)m, e_stats, t_stats, out);
    XV_LAUNCH_CHECK();
    return 0;
}
