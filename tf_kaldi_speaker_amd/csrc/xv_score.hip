// Cosine trial scoring with adaptive symmetric score normalisation (AS-norm): what ivector-subtract-global-mean | ivector-normalize-length,
// ivector-compute-dot-products and the cohort statistics of an AS-norm back end do behind the reference's extract.py, on embedding
// matrices that live on the device.  Three ops: rows centred and scaled to unit length (score_prepare), trial dot products with the
// optional normalisation (score_trials), and per row the mean / deviation of its top-k cohort scores (score_cohort_stats: the project's
// fp32 NT GEMM into a score slab, then an exact radix select per row).  No floating-point atomics and no cross-workgroup hand-over in
// these kernels (the select's histogram is integer LDS atomics: a count does not depend on the order of its increments): a result
// depends on the shape of the call only, so it is the same bits every time.  gfx950 only.
#include <algorithm>

#include "xv_common.h"
#include "xv_ew.h"
#include "xv_gemm.h"
#include "xv_rowsum.h"      // sc_row_dot and chain(d), SC_ROWS_PER_WG, sc_aligned16, sc_overlap
#include "xv_radix_key.h"   // sc_key / sc_unkey: the unsigned key whose order is the float's

#define SC_SEL_THREADS 256
#define SC_TILE_ROWS 128          // the score slab holds a whole number of GEMM row tiles

// y[r][c] = v * rsqrt(max(Σ v², 1e-12)), v = x[r][c] - mean[c], for c < d; y[r][d .. ldy) = 0.  One wave per row.  In place (y == x,
// ldy == ldx) a lane reads back exactly the elements it then overwrites, and the padding belongs to the row.
template <bool VEC, bool SUB>
__global__ __launch_bounds__(256) void score_prepare_kernel(const float* x, int rows, int d, long ldx, const float* __restrict__ mean, float* y, long ldy) {
    XV_EW_PRIORITY();
    const int r = blockIdx.x * SC_ROWS_PER_WG + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* xr = x + (long)r * ldx;
    float* yr = y + (long)r * ldy;
    const float ss = sc_row_dot<VEC, SUB>(xr, xr, mean, d, lane);
    const float inv = rsqrtf(fmaxf(ss, 1e-12f));
    if (VEC) {
        for (int q = lane; q < (int)(ldy / 4); q += XV_WAVE) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < d / 4) {
                v = *(const f32x4*)(xr + 4 * q);
                if (SUB) v -= *(const f32x4*)(mean + 4 * q);
                v *= inv;
            }
            *(f32x4*)(yr + 4 * q) = v;
        }
    } else {
        for (int c = lane; c < (int)ldy; c += XV_WAVE) {
            float v = 0.f;
            if (c < d) {
                v = xr[c];
                if (SUB) v -= mean[c];
                v *= inv;
            }
            yr[c] = v;
        }
    }
}

// out[j] = s = Σ_c e[ei[j]][c] * t[ti[j]][c], or with the row statistics 0.5 * ((s - μe) / σe + (s - μt) / σt).  One wave per trial;
// the sum is sc_row_dot's (chain(d) above).
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
    float s = sc_row_dot<VEC, false>(e + (long)a * lde, t + (long)b * ldt, nullptr, d, lane);
    if (e_stats) s = 0.5f * ((s - e_stats[2 * (long)a]) / e_stats[2 * (long)a + 1] + (s - t_stats[2 * (long)b]) / t_stats[2 * (long)b + 1]);
    if (lane == 0) out[j] = s;
}

// a double summed over the workgroup in a fixed order: butterfly inside each wave, the four wave totals added first to last
__device__ __forceinline__ double sc_block_sum(double v, double* wtot, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();      // (wtot may still be read from the call before)
    if ((tid & 63) == 0) wtot[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SC_SEL_THREADS / XV_WAVE; ++w) s += wtot[w];
    return s;
}

// stats[r] = (mean, sqrt(max(var, 1e-12))) of the k largest of the n scores of row r of the slab (k <= n).  One workgroup per row.
// Radix select of the k-th largest key, most significant byte first: each pass counts, among the elements that share the bytes already
// fixed, the next byte's 256 values in LDS; wave 0 walks the counts from the top until `want` more elements are covered, which fixes the
// byte and leaves `want` = the rank inside that bucket.  After four passes the key is the k-th largest score exactly and `want` is how
// many copies of it the top k holds (k - want elements lie strictly above).  The sums take the elements strictly above plus `want` copies
// of the threshold, so a cut through a run of equal scores is well defined; they are accumulated in double (a thread's elements in index
// order, then sc_block_sum), the variance around the mean in a second pass.  The row is streamed from the slab six times; nothing of it
// is kept in LDS, so n is not bounded here.
__global__ __launch_bounds__(SC_SEL_THREADS) void score_select_kernel(const float* __restrict__ slab, long lds, int n, int k, float* __restrict__ stats) {
    XV_EW_PRIORITY();
    __shared__ int hist[256];
    __shared__ unsigned sh_prefix;
    __shared__ int sh_want;
    __shared__ double wtot[SC_SEL_THREADS / XV_WAVE];
    const int tid = threadIdx.x;
    const float* row = slab + (long)blockIdx.x * lds;
    const int n4 = n / 4;      // (every slab row starts on a 16-byte boundary: the slab is 16-byte aligned and lds a multiple of 4)
    unsigned prefix = 0, mask = 0;
    int want = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int q = tid; q < n4; q += SC_SEL_THREADS) {
            const f32x4 v = *(const f32x4*)(row + 4 * q);
            const unsigned k0 = sc_key(v.x), k1 = sc_key(v.y), k2 = sc_key(v.z), k3 = sc_key(v.w);
            if ((k0 & mask) == prefix) atomicAdd(&hist[(k0 >> shift) & 255u], 1);
            if ((k1 & mask) == prefix) atomicAdd(&hist[(k1 >> shift) & 255u], 1);
            if ((k2 & mask) == prefix) atomicAdd(&hist[(k2 >> shift) & 255u], 1);
            if ((k3 & mask) == prefix) atomicAdd(&hist[(k3 >> shift) & 255u], 1);
        }
        if (tid < n - 4 * n4) {
            const unsigned kk = sc_key(row[4 * n4 + tid]);
            if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < XV_WAVE) {      // lane l owns the buckets 255 - 4l ... 252 - 4l, walked downwards
            int c[4], own = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; own += c[j]; }
            int incl = own;
#pragma unroll
            for (int o = 1; o < XV_WAVE; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (tid >= o) incl += up;
            }
            int above = incl - own;      // elements in the buckets of the lanes in front
            if (above < want && want <= incl) {      // exactly one lane: the buckets hold at least `want` elements together
                int digit = 255 - 4 * tid - 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (want <= above + c[j]) { digit = 255 - 4 * tid - j; break; }
                    above += c[j];
                }
                sh_prefix = prefix | ((unsigned)digit << shift);
                sh_want = want - above;
            }
        }
        __syncthreads();
        prefix = sh_prefix;
        want = sh_want;
        mask |= 255u << shift;
    }
    const float thr = sc_unkey(prefix);
    const double dthr = (double)thr;
    double acc = 0.0;
    for (int q = tid; q < n4; q += SC_SEL_THREADS) {
        const f32x4 v = *(const f32x4*)(row + 4 * q);
        if (sc_key(v.x) > prefix) acc += (double)v.x;
        if (sc_key(v.y) > prefix) acc += (double)v.y;
        if (sc_key(v.z) > prefix) acc += (double)v.z;
        if (sc_key(v.w) > prefix) acc += (double)v.w;
    }
    if (tid < n - 4 * n4) {
        const float v = row[4 * n4 + tid];
        if (sc_key(v) > prefix) acc += (double)v;
    }
    const double mean = (sc_block_sum(acc, wtot, tid) + (double)want * dthr) / (double)k;
    acc = 0.0;
    for (int q = tid; q < n4; q += SC_SEL_THREADS) {
        const f32x4 v = *(const f32x4*)(row + 4 * q);
        if (sc_key(v.x) > prefix) acc += ((double)v.x - mean) * ((double)v.x - mean);
        if (sc_key(v.y) > prefix) acc += ((double)v.y - mean) * ((double)v.y - mean);
        if (sc_key(v.z) > prefix) acc += ((double)v.z - mean) * ((double)v.z - mean);
        if (sc_key(v.w) > prefix) acc += ((double)v.w - mean) * ((double)v.w - mean);
    }
    if (tid < n - 4 * n4) {
        const float v = row[4 * n4 + tid];
        if (sc_key(v) > prefix) acc += ((double)v - mean) * ((double)v - mean);
    }
    const double var = (sc_block_sum(acc, wtot, tid) + (double)want * (dthr - mean) * (dthr - mean)) / (double)k;
    if (tid == 0) {
        stats[2 * (long)blockIdx.x] = (float)mean;
        stats[2 * (long)blockIdx.x + 1] = (float)sqrt(fmax(var, 1e-12));
    }
}

extern "C" int xv_score_prepare(void* stream, const float* x, int rows, int d, int ldx, const float* mean, float* y, int ldy) {
    XV_REQUIRE(x && y && rows > 0 && d > 0, "score_prepare: bad arguments");
    XV_REQUIRE(ldx >= d && ldy >= d, "score_prepare: a pitch is below d (d=%d ldx=%d ldy=%d)", d, ldx, ldy);
    const bool in_place = x == y && ldx == ldy;
    XV_REQUIRE(in_place || !sc_overlap(x, (size_t)(rows - 1) * ldx + d, y, (size_t)rows * ldy),
               "score_prepare: x and y overlap (in place needs y == x and the same pitch)");
    XV_REQUIRE(!mean || !sc_overlap(mean, d, y, (size_t)rows * ldy), "score_prepare: mean and y overlap");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && sc_aligned16(x) && sc_aligned16(y) && (!mean || sc_aligned16(mean));
    const dim3 grid(xv_cdiv(rows, SC_ROWS_PER_WG)), block(256);
    if (vec && mean) hipLaunchKernelGGL((score_prepare_kernel<true, true>), grid, block, 0, s, x, rows, d, (long)ldx, mean, y, (long)ldy);
    else if (vec) hipLaunchKernelGGL((score_prepare_kernel<true, false>), grid, block, 0, s, x, rows, d, (long)ldx, mean, y, (long)ldy);
    else if (mean) hipLaunchKernelGGL((score_prepare_kernel<false, true>), grid, block, 0, s, x, rows, d, (long)ldx, mean, y, (long)ldy);
    else hipLaunchKernelGGL((score_prepare_kernel<false, false>), grid, block, 0, s, x, rows, d, (long)ldx, mean, y, (long)ldy);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_score_trials(void* stream, const float* e, int lde, int ne, const float* t, int ldt, int nt, int d, const int32_t* ei,
                               const int32_t* ti, int64_t m, const float* e_stats, const float* t_stats, float* out) {
    XV_REQUIRE(e && t && ei && ti && out && ne > 0 && nt > 0 && d > 0 && m > 0, "score_trials: bad arguments");
    XV_REQUIRE(lde >= d && ldt >= d, "score_trials: a pitch is below d (d=%d lde=%d ldt=%d)", d, lde, ldt);
    XV_REQUIRE((e_stats != nullptr) == (t_stats != nullptr), "score_trials: e_stats and t_stats must both be given or both be NULL");
    XV_REQUIRE(m <= (int64_t)SC_ROWS_PER_WG * 0x7fffffff, "score_trials: too many trials in one call (%lld)", (long long)m);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = d % 4 == 0 && lde % 4 == 0 && ldt % 4 == 0 && sc_aligned16(e) && sc_aligned16(t);
    const dim3 grid((unsigned)((m + SC_ROWS_PER_WG - 1) / SC_ROWS_PER_WG)), block(256);
    if (vec) hipLaunchKernelGGL(score_trials_kernel<true>, grid, block, 0, s, e, (long)lde, t, (long)ldt, d, (const int*)ei, (const int*)ti, (long)m, e_stats, t_stats, out);
    else hipLaunchKernelGGL(score_trials_kernel<false>, grid, block, 0, s, e, (long)lde, t, (long)ldt, d, (const int*)ei, (const int*)ti, (long)m, e_stats, t_stats, out);
    XV_LAUNCH_CHECK();
    return 0;
}

// floats per slab row: the cohort size on the 16-byte grid
static size_t sc_slab_pitch(int n_cohort) { return xv_align((size_t)(n_cohort > 0 ? n_cohort : 1), 4); }

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
    // rows per slab: whole GEMM row tiles, as many as the workspace holds and as the GEMM addresses (an operand spans less than 4 GB:
    // xv_launch_gemm_nt; a pitch so long that not even one tile fits under that is refused there)
    const size_t fit = ws_bytes / (pitch * sizeof(float)) / SC_TILE_ROWS * SC_TILE_ROWS;
    const size_t span = (((size_t)1 << 32) - 1) / ((size_t)ldx * sizeof(float));
    const size_t cap = span > SC_TILE_ROWS + 1 ? (span - 1) / SC_TILE_ROWS * SC_TILE_ROWS : SC_TILE_ROWS;
    const int tile = (int)std::min(std::min(fit, cap), (size_t)1 << 20);
    const int k = top_k < n_cohort ? top_k : n_cohort;
    for (int r0 = 0; r0 < rows; r0 += tile) {
        const int m = rows - r0 < tile ? rows - r0 : tile;
        // xv_affine_forward with k = 1, segs = m, t_in = 1, except that a row pitch may exceed K; no scratch: one workgroup per tile
        XvGemmNT g = {};
        g.A = x + (size_t)r0 * ldx; g.lda = ldx; g.a_rps = 1; g.a_pitch = 1;
        g.Bt = cohort; g.ldb = ldc;
        g.C = (float*)ws; g.ldc = (long)pitch;
        g.M = m; g.N = n_cohort; g.K = kd;
        const int rc = xv_launch_gemm_nt(s, g);
        if (rc) return rc;
        hipLaunchKernelGGL(score_select_kernel, dim3(m), dim3(SC_SEL_THREADS), 0, s, (const float*)ws, (long)pitch, n_cohort, k, stats + 2 * (size_t)r0);
        XV_LAUNCH_CHECK();
    }
    return 0;
}
