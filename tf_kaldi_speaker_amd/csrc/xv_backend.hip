// The LDA / PLDA back end behind extraction (egs/voxceleb/v1/run.sh stages 10-11, egs/sre/v1/run.sh): the device side of ivector-mean
// (per-speaker averages), ivector-compute-lda / ivector-compute-plda (the scatter statistics), ivector-subtract-global-mean and
// ivector-plda-scoring (the normalisation of a transformed vector and the per-trial log-likelihood ratio) on embedding matrices that
// live on the device.  The eigendecompositions and the EM run on the host in fp64 (misc/backend.py); the affine maps are the project's
// fp32 NT GEMM (xv_affine_forward).  Five ops: group_means, center, scatter (the project's fp32 TN GEMM per row block, the blocks'
// slabs added in double), plda_normalize, plda_trials.  No floating-point atomics and no cross-workgroup hand-over in these kernels: a
// result depends on the shape of the call only, so it is the same bits every time.  gfx950 only.
//
// Error budget of plda_trials (tests/test_gpu_backend.py): per column a lane runs
//     diff = fma(-a, e, t); acc = fma(-0.5 * (iv * diff), diff, acc); acc = fma(0.5 * (g * t), t, acc)
// - three roundings inside the first term (diff counts twice in diff^2, iv * diff once), one inside the second, and two adds on the chain,
// which is 2 * (chain(d) - 6) + 6 = 2 chain(d) - 6 adds long (sc_row_sum of xv_rowsum.h calls a lane's term at most chain(d) - 6 times, this
// term puts two fmas on acc, and the butterfly adds six; both forms interleaved in ONE sum, so a partial sum is bounded by the sum of the
// |terms|, not by either quadratic form alone).  With the final k0 + s that is at most
//     (2 chain(d) - 2) EPS * sum_c (|0.5 iv (t - a e)^2| + |0.5 g t^2|) + EPS |k0|
// to first order, inside the 2 * (2 chain(d) + 6) EPS * sum + EPS |k0| the test asserts.
#include <algorithm>

#include "xv_common.h"
#include "xv_ew.h"
#include "xv_gemm.h"
#include "xv_rowsum.h"
#include "xv_score_launch.h"

#define BE_BLOCK_ROWS 8192        // rows per scatter block: the longest fp32 add chain of a scatter element, whatever n is

// mean64[g][c] = (sum of x[rows[i]][c] over i in [offsets[g], offsets[g + 1]), added in list order in double) / count; mean32 its fp32
// rounding, columns d .. ldm zero.  One thread per (group, column), the column fastest: a wave gathers 64 neighbouring floats of one row.
__global__ __launch_bounds__(256) void backend_group_means_kernel(const float* __restrict__ x, long ldx, int d, const long* __restrict__ offsets,
                                                                  const int* __restrict__ rows, int groups, double* __restrict__ mean64,
                                                                  float* __restrict__ mean32, long ldm) {
    XV_EW_PRIORITY();
    const int cols = mean32 ? (int)ldm : d;      // (ldm >= d: the padding columns have a thread of their own)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)groups * cols) return;
    const int g = (int)(idx / cols), c = (int)(idx - (long)g * cols);
    if (c >= d) {
        mean32[(long)g * ldm + c] = 0.f;
        return;
    }
    const long i0 = offsets[g], i1 = offsets[g + 1];
    double acc = 0.0;
    for (long i = i0; i < i1; ++i) acc += (double)x[(long)rows[i] * ldx + c];
    const double m = acc / (double)(i1 - i0);
    mean64[(long)g * d + c] = m;
    if (mean32) mean32[(long)g * ldm + c] = (float)m;
}

// y[r][c] = x[r][c] - mean[c] (mean == nullptr: x[r][c]) for c < d, 0 for d <= c < ldy: the fp32 subtraction of score_prepare, without the scaling
__global__ __launch_bounds__(256) void backend_center_kernel(const float* x, long ldx, int rows, int d, const float* __restrict__ mean, float* y,
                                                             long ldy) {
    XV_EW_PRIORITY();
    const long total = (long)rows * ldy;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / ldy;
        const int c = (int)(idx - r * ldy);
        float v = 0.f;
        if (c < d) {
            v = x[r * ldx + c];
            if (mean) v -= mean[c];
        }
        y[idx] = v;
    }
}

// c64[i][j] (+)= sum over the block's slabs, in slab order, of P[z][min(i, j)][max(i, j)], in double; first: the sum starts at 0.
// Only the upper triangle of a slab is read, so the result is bit-symmetric by construction.  One thread per element.
__global__ __launch_bounds__(256) void backend_slab_add_kernel(const float* __restrict__ P, int slabs, int dp, int d, int first, double* __restrict__ c64) {
    XV_EW_PRIORITY();
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)d * d) return;
    const int i = (int)(idx / d), j = (int)(idx - (long)i * d);
    const float* src = P + (long)min(i, j) * dp + max(i, j);
    double acc = first ? 0.0 : c64[idx];
    for (int z = 0; z < slabs; ++z) acc += (double)src[(long)z * dp * dp];
    c64[idx] = acc;
}

// out[r][c] = u[r][c] * sqrt(d / sum_c u[r][c]^2 / (psi[c] + 1 / n_r)) for c < d, 0 for d <= c < ldo.  One wave per row; the sum is
// sc_row_sum's (chain(d)).  A row whose sum is 0 stays 0.  In place a lane reads back exactly the elements it then overwrites (sc_row_store).
template <bool VEC>
__global__ __launch_bounds__(256) void backend_plda_normalize_kernel(const float* u, int rows, int d, long ldu, const float* __restrict__ psi,
                                                                     const int* __restrict__ n_utts, float* out, long ldo) {
    XV_EW_PRIORITY();
    const int r = blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* ur = u + (long)r * ldu;
    float* yr = out + (long)r * ldo;
    const float inv_n = n_utts ? 1.0f / (float)n_utts[r] : 1.0f;
    const float ss = sc_row_sum<VEC>(d, lane, [inv_n](float acc, float v, float p) { return fmaf(v, v / (p + inv_n), acc); }, ur, psi);
    const float scale = ss > 0.f ? sqrtf((float)d / ss) : 0.f;
    sc_row_store<VEC>(yr, ldo, d, lane, [scale](auto v) { return v * scale; }, ur);
}

// out[j] = k0[q] + sum_c (-0.5 iv[q][c] (t_c - a[q][c] e_c)^2 + 0.5 g[c] t_c^2), e = enrol row ei[j], t = test row ti[j], q = nidx[ei[j]];
// coef[q] = (a[ldc], iv[ldc]).  One wave per trial, the lanes and the butterfly of sc_row_sum, the two forms interleaved in one sum (the
// budget is in the header of this file).  No division, no logarithm: the host built the tables in double.
template <bool VEC>
__global__ __launch_bounds__(256) void backend_plda_trials_kernel(const float* __restrict__ e, long lde, const float* __restrict__ t, long ldt, int d,
                                                                  const int* __restrict__ ei, const int* __restrict__ ti, long m,
                                                                  const int* __restrict__ nidx, const float* __restrict__ coef, long ldc,
                                                                  const float* __restrict__ g, const float* __restrict__ k0,
                                                                  float* __restrict__ out) {
    XV_EW_PRIORITY();
    const long j = (long)blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= m) return;
    const int a_row = ei[j], b_row = ti[j], q = nidx[a_row];
    const float* er = e + (long)a_row * lde;
    const float* tr = t + (long)b_row * ldt;
    const float* ca = coef + (long)q * 2 * ldc;
    const float* ci = ca + ldc;
    const float s = sc_row_sum<VEC>(d, lane, [](float acc, float ec, float tc, float ac, float ic, float gc) {
        const float diff = fmaf(-ac, ec, tc);
        acc = fmaf(-0.5f * (ic * diff), diff, acc);
        return fmaf(0.5f * (gc * tc), tc, acc);
    }, er, tr, ca, ci, g);
    if (lane == 0) out[j] = k0[q] + s;
}

extern "C" int xv_backend_group_means(void* stream, const float* x, int n, int ldx, int d, const int64_t* offsets, const int32_t* rows, int groups,
                                      int64_t total, double* mean64, float* mean32, int ldm) {
    XV_REQUIRE(d > 0, "backend_group_means: d must be positive (got %d)", d);
    XV_REQUIRE(groups > 0, "backend_group_means: an empty list of groups (groups=%d)", groups);
    XV_REQUIRE(total >= groups, "backend_group_means: %lld rows listed for %d groups: a group would be empty", (long long)total, groups);
    XV_REQUIRE(x && offsets && rows && mean64 && n > 0, "backend_group_means: bad arguments");
    XV_REQUIRE(ldx >= d && (!mean32 || ldm >= d), "backend_group_means: a pitch is below d (d=%d ldx=%d ldm=%d)", d, ldx, ldm);
    XV_REQUIRE(((uintptr_t)mean64 % 8) == 0 && ((uintptr_t)offsets % 8) == 0, "backend_group_means: mean64 and offsets must be 8-byte aligned");
    const long cols = mean32 ? ldm : d;
    XV_REQUIRE((long)groups * cols < ((long)1 << 39), "backend_group_means: too many (group, column) pairs in one call");
    hipLaunchKernelGGL(backend_group_means_kernel, dim3((unsigned)(((long)groups * cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx,
                       d, (const long*)offsets, (const int*)rows, groups, mean64, mean32, (long)ldm);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_backend_center(void* stream, const float* x, int rows, int d, int ldx, const float* mean, float* y, int ldy) {
    XV_REQUIRE(d > 0, "backend_center: d must be positive (got %d)", d);
    XV_REQUIRE(x && y && rows > 0, "backend_center: bad arguments");
    XV_REQUIRE(ldx >= d && ldy >= d, "backend_center: a pitch is below d (d=%d ldx=%d ldy=%d)", d, ldx, ldy);
    if (const int rc = sc_check_row_out("backend_center", "x", x, ldx, "y", y, ldy, rows, d, "mean", mean)) return rc;
    hipLaunchKernelGGL(backend_center_kernel, dim3(grid_for((long)rows * ldy, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, rows, d, mean,
                       y, (long)ldy);
    XV_LAUNCH_CHECK();
    return 0;
}

// the scatter's workspace: [the centred copy of one row block: block rows x dp floats][the block's slabs: splits x dp x dp floats]
static size_t be_copy_floats(int n, int dp) { return xv_align((size_t)std::min(n, BE_BLOCK_ROWS) * dp, 64); }
static int be_max_splits(int n, int dp) {
    int s = xv_tn_splits(dp, dp, std::min(n, BE_BLOCK_ROWS));
    if (n > BE_BLOCK_ROWS && n % BE_BLOCK_ROWS) s = std::max(s, xv_tn_splits(dp, dp, n % BE_BLOCK_ROWS));
    return s;
}

extern "C" size_t xv_backend_scatter_workspace_bytes(int n, int d) {
    if (n <= 0 || d <= 0) return 0;
    const int dp = (int)xv_align(d, 4);
    return (be_copy_floats(n, dp) + (size_t)be_max_splits(n, dp) * dp * dp) * sizeof(float);
}

extern "C" int xv_backend_scatter(void* stream, const float* x, int n, int d, int ldx, const float* mean, double* c64, void* ws, size_t ws_bytes) {
    XV_REQUIRE(d > 0, "backend_scatter: d must be positive (got %d)", d);
    XV_REQUIRE(x && c64 && n > 0, "backend_scatter: bad arguments");
    XV_REQUIRE(ldx >= d, "backend_scatter: the pitch is below d (d=%d ldx=%d)", d, ldx);
    XV_REQUIRE(((uintptr_t)c64 % 8) == 0, "backend_scatter: c64 must be 8-byte aligned");
    const int dp = (int)xv_align(d, 4);
    const size_t slab = (size_t)dp * dp * sizeof(float), need = xv_backend_scatter_workspace_bytes(n, d);
    XV_REQUIRE(ws && sc_aligned16(ws) && ws_bytes >= need,
               "backend_scatter: workspace of %zu bytes, %zu needed (the centred row block and the GEMM's slabs of %zu bytes each, 16-byte aligned)",
               ws_bytes, need, slab);
    hipStream_t s = (hipStream_t)stream;
    float* copy = (float*)ws;
    float* slabs = copy + be_copy_floats(n, dp);
    // rows that are a GEMM operand as they stand (nothing to subtract, no padding to zero, on the 16-byte grid) are not copied; the copy is
    // exact, so the bits do not depend on which way a call goes
    const bool direct = !mean && d == dp && ldx % 4 == 0 && sc_aligned16(x);
    for (int r0 = 0; r0 < n; r0 += BE_BLOCK_ROWS) {
        const int m = std::min(n - r0, BE_BLOCK_ROWS);
        const float* a = x + (size_t)r0 * ldx;
        long lda = ldx;
        if (!direct) {
            hipLaunchKernelGGL(backend_center_kernel, dim3(grid_for((long)m * dp, 256, 8192)), dim3(256), 0, s, a, (long)ldx, m, d, mean, copy, (long)dp);
            XV_LAUNCH_CHECK();
            a = copy;
            lda = dp;
        }
        // xv_affine_wgrad with k = 1, segs = m, t_in = 1 and the block on both sides; the slab sum is ours (in double)
        XvGemmTN g = {};
        g.A = a; g.lda = lda; g.a_rps = 1; g.a_pitch = 1;
        g.B = a; g.ldb = lda; g.b_rps = 1; g.b_pitch = 1;
        g.M = dp; g.N = dp; g.R = m;
        g.splits = xv_tn_splits(dp, dp, m);
        g.P = slabs;
        const int rc = xv_launch_gemm_tn(s, g);
        if (rc) return rc;
        hipLaunchKernelGGL(backend_slab_add_kernel, dim3((unsigned)(((long)d * d + 255) / 256)), dim3(256), 0, s, (const float*)slabs, g.splits, dp, d,
                           r0 == 0 ? 1 : 0, c64);
        XV_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int xv_backend_plda_normalize(void* stream, const float* u, int rows, int d, int ldu, const float* psi, const int32_t* n_utts, float* out,
                                         int ldo) {
    XV_REQUIRE(d > 0, "backend_plda_normalize: d must be positive (got %d)", d);
    XV_REQUIRE(u && psi && out && rows > 0, "backend_plda_normalize: bad arguments");
    XV_REQUIRE(ldu >= d && ldo >= d, "backend_plda_normalize: a pitch is below d (d=%d ldu=%d ldo=%d)", d, ldu, ldo);
    if (const int rc = sc_check_row_out("backend_plda_normalize", "u", u, ldu, "out", out, ldo, rows, d, "psi", psi)) return rc;
    return sc_launch_rows(backend_plda_normalize_kernel<true>, backend_plda_normalize_kernel<false>, sc_vec_ok(d, {ldu, ldo}, {u, out, psi}), rows, nullptr,
                          (hipStream_t)stream, u, rows, d, ldu, psi, n_utts, out, ldo);
}

extern "C" int xv_backend_plda_trials(void* stream, const float* e, int lde, int ne, const float* t, int ldt, int nt, int d, const int32_t* ei,
                                      const int32_t* ti, int64_t m, const int32_t* nidx, const float* coef, int ldc, int n_distinct, const float* g,
                                      const float* k0, float* out) {
    XV_REQUIRE(d > 0, "backend_plda_trials: d must be positive (got %d)", d);
    XV_REQUIRE(e && t && ei && ti && nidx && coef && g && k0 && out && ne > 0 && nt > 0 && m > 0 && n_distinct > 0, "backend_plda_trials: bad arguments");
    XV_REQUIRE(lde >= d && ldt >= d && ldc >= d, "backend_plda_trials: a pitch is below d (d=%d lde=%d ldt=%d ldc=%d)", d, lde, ldt, ldc);
    return sc_launch_rows(backend_plda_trials_kernel<true>, backend_plda_trials_kernel<false>, sc_vec_ok(d, {lde, ldt, ldc}, {e, t, coef, g}), m,
                          "backend_plda_trials: too many trials in one call (%lld)", (hipStream_t)stream, e, lde, t, ldt, d, ei, ti, m, nidx, coef, ldc, g, k0,
                          out);
}
