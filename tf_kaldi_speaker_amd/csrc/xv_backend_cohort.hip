// Cohort statistics of PLDA scores, for AS-norm behind the PLDA back end (egs/sre/v1/run.sh scores with ivector-plda-scoring; the
// normalisation is the one xv_score.hip applies to cosine scores): per row the mean / deviation of its top-k log-likelihood ratios against
// the cohort rows.  xv_backend_plda_trials gathers two rows per score, which is hopeless for rows x n_cohort scores; here the ratio of a
// model row e (n utterances, table index q) against a one-utterance test row t is taken in its factored form
//     LLR(e, t) = R(e) + C_q(t) + sum_c (iv_q[c] a_q[c] e_c) t_c,
//     R(e)   = k0[q] - 0.5 sum_c iv_q[c] a_q[c]^2 e_c^2,        C_q(t) = 0.5 sum_c (g[c] - iv_q[c]) t_c^2
// (a, iv, g, k0: the tables of plda_coefficients, misc/backend.py) - one GEMM plus a row term and a column term.  For n = 1 the ratio is
// symmetric in (e, t), so a test row enters as a one-utterance model.  Per call: the column terms of every (q, cohort row) once; per row
// tile: the fold kernel (the GEMM operand xs = iv a x and R), the project's fp32 NT GEMM xs . cohort^T into the score slab
// (xv_launch_gemm_nt, as xv_score_cohort_stats calls it), and the exact radix select of xv_select.h over
//     v(r, j) = (slab[r][j] + C_q[j]) + R[r]
// - one parenthesised sum of two plain fp32 adds, written once (PcRow) and so the same bits in each of the select's six passes.  No
// floating-point atomics and no cross-workgroup hand-over: a result depends on the shape of the call only, so it is the same bits every time.
// gfx950 only.
//
// Roofs (no rate is claimed): column-term and fold kernels are HBM-bound (n_distinct x n_cohort x d and rows x d floats read, rows x kd
// written); the GEMM is MFMA-bound at 2 rows n_cohort d FLOP; the selection streams 6 rows n_cohort 4 bytes of the slab, the column vector
// of a row's q (n_cohort floats, shared by every row of that q) coming out of L2.
//
// Error budget of v(r, j) against the same fp32 tables in exact arithmetic (tests/test_gpu_plda_cohort.py), EPS = 2^-24, kd = d rounded up
// to 4, chain(d) of xv_rowsum.h:
//   GEMM      xs_c carries two roundings (iv a, then times x); each of the kd steps of a sum of products, in whatever order the GEMM takes
//             its K, rounds at most twice (the product and the add; once where the unit fuses them), every partial sum bounded by
//             sum_c |xs_c t_c|: (2 kd + 2) EPS sum_c |xs_c t_c|
//   C_q(t_j)  a term 0.5 ((g - iv) t) t carries two roundings and the fma's; the chain is sc_row_sum's: (chain(d) + 2) EPS sum_c |term|
//   R(x_r)    a term (a xs) x carries xs's two roundings and one more, the chain the same (the fold kernel walks sc_row_sum's lanes,
//             one fma on acc per column), then one fma -0.5 S + k0:
//             (chain(d) + 3) EPS sum_c |term| + EPS |R|
//   v         two adds: 2 EPS (|slab| + |C| + |R|)
// together at most c1 EPS (sum |xs t| + sum |terms of C| + sum |terms of R| + |k0|) with c1 = max(2 kd + 2, chain(d) + 3) + 4: the three
// roundings above that every part meets, and one more for the second order (c1 EPS < 1e-4, so (1 + EPS)^c1 - 1 < (c1 + 1) EPS).  The test
// asserts exactly this c1.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_gemm.h"
#include "xv_rowsum.h"
#include "xv_score_launch.h"
#include "xv_select.h"

// ct[q][j] = 0.5 sum_c (g[c] - iv_q[c]) t_j[c]^2: one wave per (q, j).  coef[q] = (a[ldk], iv[ldk]).  The sum is sc_row_sum's.
template <bool VEC>
__global__ __launch_bounds__(256) void plda_cohort_colterm_kernel(const float* __restrict__ cohort, long ldc, int n_cohort, int d,
                                                                  const float* __restrict__ coef, long ldk, int n_distinct,
                                                                  const float* __restrict__ g, float* __restrict__ ct, long pitch) {
    XV_EW_PRIORITY();
    const long idx = (long)blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (idx >= (long)n_distinct * n_cohort) return;
    const int q = (int)(idx / n_cohort), j = (int)(idx - (long)q * n_cohort);
    const float* tr = cohort + (long)j * ldc;
    const float* ci = coef + ((long)q * 2 + 1) * ldk;
    const float s = sc_row_sum<VEC>(d, lane, [](float acc, float tc, float ic, float gc) { return fmaf(0.5f * ((gc - ic) * tc), tc, acc); }, tr, ci, g);
    if (lane == 0) ct[(long)q * pitch + j] = s;
}

// xs[r][c] = (iv_q[c] a_q[c]) x[r][c] for c < d, 0 for d <= c < kd (the GEMM operand); rterm[r] = k0[q] - 0.5 sum_c (a_q[c] xs[r][c]) x[r][c];
// q = nidx[r] (nullptr: 0).  One wave per row.  The lanes and the butterfly are sc_row_sum's (xv_rowsum.h) written out: the pass that sums
// also stores xs, and its scalar form runs on to kd for the padding, which is neither that walker nor sc_row_store.
template <bool VEC>
__global__ __launch_bounds__(256) void plda_cohort_fold_kernel(const float* __restrict__ x, long ldx, int rows, int d, const int* __restrict__ nidx,
                                                               const float* __restrict__ coef, long ldk, const float* __restrict__ k0,
                                                               float* __restrict__ xs, int kd, float* __restrict__ rterm) {
    XV_EW_PRIORITY();
    const int r = blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const int q = nidx ? nidx[r] : 0;
    const float* xr = x + (long)r * ldx;
    const float* ca = coef + (long)q * 2 * ldk;
    const float* ci = ca + ldk;
    float* yr = xs + (long)r * kd;
    float acc = 0.f;
    if (VEC) {      // (d % 4 == 0: kd == d, no padding column)
        for (int p = lane; p < d / 4; p += XV_WAVE) {
            const f32x4 xv = *(const f32x4*)(xr + 4 * p), av = *(const f32x4*)(ca + 4 * p), iv = *(const f32x4*)(ci + 4 * p);
            f32x4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                y[k] = (iv[k] * av[k]) * xv[k];
                acc = fmaf(av[k] * y[k], xv[k], acc);
            }
            *(f32x4*)(yr + 4 * p) = y;
        }
    } else {
        for (int c = lane; c < kd; c += XV_WAVE) {
            float y = 0.f;
            if (c < d) {
                const float xc = xr[c];
                y = (ci[c] * ca[c]) * xc;
                acc = fmaf(ca[c] * y, xc, acc);
            }
            yr[c] = y;
        }
    }
    const float s = wave_sum(acc);
    if (lane == 0) rterm[r] = fmaf(-0.5f, s, k0[q]);
}

// the element of the PLDA selection for the row of this workgroup: v(j) = (slab[j] + ct[j]) + rt - stated here once, a pure function of j.
// sc_select_kernel<PcRow, ...> (xv_select.h) hands over the slab row and the launch's extra arguments: the column terms [n_distinct][pitch]
// (their pitch is the slab's), the rows' table entries (nullptr: 0) and row terms.  Slab and ct rows start on 16-byte boundaries.
struct PcRow {
    const float* slab;      // the row's GEMM sums
    const float* ct;        // the column terms of the row's q
    float rt;               // the row term
    __device__ __forceinline__ PcRow(const float* row, long pitch, const float* cterms, const int* nidx, const float* rterm)
        : slab(row), ct(cterms + (long)(nidx ? nidx[blockIdx.x] : 0) * pitch), rt(rterm[blockIdx.x]) {}
    __device__ __forceinline__ f32x4 load4(int q) const { return (*(const f32x4*)(slab + 4 * q) + *(const f32x4*)(ct + 4 * q)) + rt; }
    __device__ __forceinline__ float load1(int i) const { return (slab[i] + ct[i]) + rt; }
};

// The column terms of every (q, cohort row) and the fold of m rows: the two launches the cohort op and the dense op share.  too_many: the
// op's refusal of more pairs than one grid takes (sc_launch_rows).
static int pc_launch_colterm(hipStream_t s, const char* too_many, const float* cohort, int ldc, int n_cohort, int d, const float* coef, int ldk,
                             int n_distinct, const float* g, float* ct, size_t pitch) {
    return sc_launch_rows(plda_cohort_colterm_kernel<true>, plda_cohort_colterm_kernel<false>, sc_vec_ok(d, {ldc, ldk}, {cohort, coef, g}),
                          (long)n_distinct * n_cohort, too_many, s, cohort, ldc, n_cohort, d, coef, ldk, n_distinct, g, ct, pitch);
}
static int pc_launch_fold(hipStream_t s, const float* x, int ldx, int m, int d, const int* nidx, const float* coef, int ldk, const float* k0, float* xs,
                          int kd, float* rterm) {
    return sc_launch_rows(plda_cohort_fold_kernel<true>, plda_cohort_fold_kernel<false>, sc_vec_ok(d, {ldx, ldk}, {x, coef}), m, nullptr, s, x, ldx, m, d,
                          nidx, coef, ldk, k0, xs, kd, rterm);
}

// Workspace of the cohort op, as float offsets: [ct: n_distinct x pitch][slab: tile x pitch][xs: tile x kd][rterm: tile], pitch = n_cohort
// rounded up to 4, kd = d rounded up to 4, tile = the rows of one round, a multiple of 128 - so every part starts on a 16-byte boundary.
struct PcLayout {
    size_t pitch, kd, slab, xs, rterm, total;      // (ct is at 0)
    PcLayout(size_t tile, int n_cohort, int d, int n_distinct)
        : pitch(sc_slab_pitch(n_cohort)), kd(xv_align(d > 0 ? d : 1, 4)), slab((size_t)(n_distinct > 0 ? n_distinct : 1) * pitch),
          xs(slab + tile * pitch), rterm(xs + tile * kd), total(rterm + tile) {}
    size_t rows_that_fit(size_t floats) const { return (floats - slab) / (pitch + kd + 1); }      // (floats >= slab)
};

extern "C" size_t xv_backend_plda_cohort_workspace_bytes(int rows, int n_cohort, int d, int n_distinct) {
    return PcLayout(xv_align((size_t)(rows > 0 ? rows : 1), SC_TILE_ROWS), n_cohort, d, n_distinct).total * sizeof(float);
}

extern "C" int xv_backend_plda_cohort_stats(void* stream, const float* x, int ldx, int rows, const int32_t* nidx, const float* cohort, int ldc,
                                            int n_cohort, int d, const float* coef, int ldcoef, int n_distinct, const float* g, const float* k0,
                                            int top_k, float* stats, void* ws, size_t ws_bytes) {
    XV_REQUIRE(top_k > 0, "backend_plda_cohort_stats: top_k must be positive (got %d)", top_k);
    XV_REQUIRE(n_cohort > 0, "backend_plda_cohort_stats: n_cohort must be positive (got %d)", n_cohort);
    XV_REQUIRE(d > 0, "backend_plda_cohort_stats: d must be positive (got %d)", d);
    XV_REQUIRE(x && cohort && coef && g && k0 && stats && rows > 0 && n_distinct > 0, "backend_plda_cohort_stats: bad arguments");
    const int kd = (int)xv_align(d, 4);      // the GEMM's K: columns d .. kd of the cohort rows are read (plda_normalize wrote them as zero)
    XV_REQUIRE(ldx >= kd && ldc >= kd, "backend_plda_cohort_stats: both pitches must reach d rounded up to 4 (d=%d ldx=%d ldc=%d)", d, ldx, ldc);
    XV_REQUIRE(ldcoef >= d, "backend_plda_cohort_stats: the pitch of coef is below d (d=%d ldcoef=%d)", d, ldcoef);
    // (what the GEMM would refuse, asked here so that a refusal comes before the first launch)
    XV_REQUIRE(ldc % 4 == 0 && sc_aligned16(cohort), "backend_plda_cohort_stats: the cohort must be a GEMM operand (pitch a multiple of 4, 16-byte aligned; ldc=%d)", ldc);
    const PcLayout one(SC_TILE_ROWS, n_cohort, d, n_distinct);
    XV_REQUIRE(ws && sc_aligned16(ws) && ws_bytes / sizeof(float) >= one.total,
               "backend_plda_cohort_stats: workspace of %zu bytes, the column terms and at least one %d-row tile need %zu (16-byte aligned)", ws_bytes,
               SC_TILE_ROWS, one.total * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    const int tile = sc_tile_rows(one.rows_that_fit(ws_bytes / sizeof(float)), kd);
    const PcLayout at(tile, n_cohort, d, n_distinct);
    float *ct = (float*)ws, *slab = ct + at.slab, *xs = ct + at.xs, *rterm = ct + at.rterm;
    const int k = top_k < n_cohort ? top_k : n_cohort;
    if (const int rc = pc_launch_colterm(s, "backend_plda_cohort_stats: too many (count, cohort row) pairs in one call (%lld)", cohort, ldc, n_cohort, d, coef,
                                         ldcoef, n_distinct, g, ct, at.pitch))
        return rc;
    for (int r0 = 0; r0 < rows; r0 += tile) {
        const int m = rows - r0 < tile ? rows - r0 : tile;
        const int* nr = nidx ? nidx + r0 : nullptr;
        if (const int rc = pc_launch_fold(s, x + (size_t)r0 * ldx, ldx, m, d, nr, coef, ldcoef, k0, xs, kd, rterm)) return rc;
        // xv_score_cohort_stats's GEMM, on the folded rows
        if (const int rc = sc_gemm_nt(s, xs, kd, cohort, ldc, slab, (long)at.pitch, m, n_cohort, kd)) return rc;
        hipLaunchKernelGGL((sc_select_kernel<PcRow, const float*, const int*, const float*>), dim3(m), dim3(SC_SEL_THREADS), 0, s, (const float*)slab,
                           (long)at.pitch, n_cohort, k, stats + 2 * (size_t)r0, (const float*)ct, nr, (const float*)rterm);
        XV_LAUNCH_CHECK();
    }
    return 0;
}

// ---- the dense matrix of one recording (xv_backend_plda_dense): the same factored ratio, every pair written instead of selected ----

// out[r][j] = (out[r][j] + ct[j]) + rt[r] in place over the GEMM's sums: PcRow::load1's expression with the single table entry.  One
// thread per element, a row of workgroups per matrix row; out's pitch and base are the caller's (a view into a packed buffer), so the
// accesses are single floats.
__global__ __launch_bounds__(256) void plda_dense_finish_kernel(float* out, long ldo, int n, const float* __restrict__ ct, const float* __restrict__ rterm) {
    XV_EW_PRIORITY();
    const int j = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (j >= n) return;
    float* o = out + (long)r * ldo + j;
    *o = (*o + ct[j]) + rterm[r];
}

// Workspace of the dense op, as float offsets: [ct: pitch][xs: n x kd][rterm: n], pitch = n rounded up to 4 - every part starts on a 16-byte
// boundary.
struct PdLayout {
    size_t pitch, kd, xs, rterm, total;      // (ct is at 0)
    PdLayout(int n, int d)
        : pitch(sc_slab_pitch(n)), kd(xv_align(d > 0 ? d : 1, 4)), xs(pitch), rterm(xs + (size_t)(n > 0 ? n : 1) * kd),
          total(rterm + xv_align(n > 0 ? n : 1, 4)) {}
};

extern "C" size_t xv_backend_plda_dense_workspace_bytes(int n, int d) { return PdLayout(n, d).total * sizeof(float); }

extern "C" int xv_backend_plda_dense(void* stream, const float* x, int ldx, int n, int d, const float* coef, int ldk, const float* g, const float* k0,
                                     float* out, int ldo, void* ws, size_t ws_bytes) {
    XV_REQUIRE(n > 0, "backend_plda_dense: n must be positive (got %d)", n);
    XV_REQUIRE(d > 0, "backend_plda_dense: d must be positive (got %d)", d);
    XV_REQUIRE(x && coef && g && k0 && out, "backend_plda_dense: bad arguments");
    const int kd = (int)xv_align(d, 4);      // the GEMM's K: columns d .. kd of the rows are read (plda_normalize wrote them as zero)
    XV_REQUIRE(ldx >= kd, "backend_plda_dense: the pitch must reach d rounded up to 4 (d=%d ldx=%d)", d, ldx);
    XV_REQUIRE(ldk >= d, "backend_plda_dense: the pitch of coef is below d (d=%d ldk=%d)", d, ldk);
    XV_REQUIRE(ldo >= n, "backend_plda_dense: the pitch of out is below n (n=%d ldo=%d)", n, ldo);
    XV_REQUIRE(ldx % 4 == 0 && sc_aligned16(x), "backend_plda_dense: the rows must be a GEMM operand (pitch a multiple of 4, 16-byte aligned; ldx=%d)", ldx);
    XV_REQUIRE(n <= 65535, "backend_plda_dense: too many rows in one call (%d)", n);
    const PdLayout at(n, d);
    XV_REQUIRE(ws && sc_aligned16(ws) && ws_bytes >= at.total * sizeof(float), "backend_plda_dense: workspace of %zu bytes, %zu needed (16-byte aligned)",
               ws_bytes, at.total * sizeof(float));
    XV_REQUIRE(!sc_overlap(x, (size_t)(n - 1) * ldx + kd, out, (size_t)(n - 1) * ldo + n), "backend_plda_dense: x and out overlap");
    hipStream_t s = (hipStream_t)stream;
    float *ct = (float*)ws, *xs = ct + at.xs, *rterm = ct + at.rterm;
    // the column terms and the fold of plda_cohort_stats with n_distinct = 1 and the rows as their own cohort (n <= 65535 pairs: no refusal)
    if (const int rc = pc_launch_colterm(s, nullptr, x, ldx, n, d, coef, ldk, 1, g, ct, at.pitch)) return rc;
    if (const int rc = pc_launch_fold(s, x, ldx, n, d, nullptr, coef, ldk, k0, xs, kd, rterm)) return rc;
    if (const int rc = sc_gemm_nt(s, xs, kd, x, ldx, out, ldo, n, n, kd)) return rc;
    hipLaunchKernelGGL(plda_dense_finish_kernel, dim3(xv_cdiv(n, 256), n), dim3(256), 0, s, out, (long)ldo, n, (const float*)ct, (const float*)rterm);
    XV_LAUNCH_CHECK();
    return 0;
}
