// Pairwise loss heads (model/loss.py:358-705), fp32: the semi-hard triplet loss on Euclidean distances, the angular triplet loss
// ("all" / "hard" mining, asoftmax / additive / arc margin on the positive side) on cosine similarities, and the end-to-end validation
// loss.  All three read one matrix, G = X X^T:
//   pair_gemm_kernel<true>    G = X X^T; G_ij and G_ji sum the same products in the same order, so G is symmetric to the bit
//   pair_rows_kernel<KIND>    one workgroup per anchor row: the row of the pair matrix and the labels in LDS, the mining scan, the row of
//                             the gradient d L / d (pair matrix before clip / max) WITHOUT the normaliser, and the row's (sum, counts)
//   pair_finish_kernel        the B partials in index order -> loss, stats, 1 / normaliser (stays on the device for the backward)
//   pair_sym_kernel           A = scale * (dG + dG^T) with the chain through the row norms folded into the diagonal
//   pair_gemm_kernel<false>   d X = A X
//   e2e_speaker_kernel / e2e_rows_kernel / e2e_finish_kernel   the validation loss from the same G
// and, further down, the GE2E training loss (model/loss.py:903-982) on the same G and the same two products:
//   ge2e_rows_kernel<TYPE> / ge2e_finish_kernel / ge2e_q_kernel
// The two products are kernels of this unit and not xv_launch_gemm_nt / _tn: B = 8 .. 1024 rows against the 128-row tiles and the
// split-K slabs of the launchers, and G must be symmetric to the bit.  No atomics; every sum has a fixed order, so
// two calls give the same bits.  Ties in a min / max: the lowest index takes the whole gradient.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"

namespace {

#define TP_MAX_B 1024
#define TP_Q 4              // columns per thread of a 256-thread row workgroup: j = tid + 256 q
#define TP_EPS 1e-12f       // the epsilon of l2_scaling / pairwise_cos_similarity (on the squared norm), and the "positive triplet" threshold

enum { TP_SEMIHARD = 0, TP_ALL = 1, TP_HARD = 2 };

struct TpLayout { size_t g, dp, a, part, scal, total; int bp; };
static TpLayout tp_layout(int b) {
    TpLayout l;
    l.bp = (b + 3) / 4 * 4;
    const size_t m = (size_t)b * l.bp;
    l.g = 0; l.dp = m; l.a = 2 * m; l.part = 3 * m; l.scal = l.part + 4 * (size_t)l.bp; l.total = l.scal + 8;
    return l;
}

// C[i][n] = sum_k A[i][k] * (NT ? Bm[n][k] : Bm[k][n]); 64 x 64 tile, 256 threads x (4 x 4), k in steps of 16 in ascending order, each step summed on its own.
// Rows, columns and k outside M, N, K read as 0; every pitch is a multiple of 4 floats.  Quads are whole: a row of A holds K rounded up to 4
// floats (NT: of Bm too), and C is written up to N rounded up to 4.
template <bool NT>
__global__ __launch_bounds__(256) void pair_gemm_kernel(const float* __restrict__ A, int lda, const float* __restrict__ Bm, int ldb, int M, int N,
                                                        int K, float* __restrict__ C, int ldc) {
    XV_EW_PRIORITY();
    __shared__ float sa[16][68], sb[16][68];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        {   // A tile: 64 rows x 16 k, one quad per thread, stored k-major
            const int row = tid >> 2, kq = (tid & 3) * 4;
            f32x4 v = f32x4{0, 0, 0, 0};
            if (i0 + row < M && k0 + kq < K) v = *(const f32x4*)(A + (long)(i0 + row) * lda + k0 + kq);
            sa[kq + 0][row] = v.x; sa[kq + 1][row] = v.y; sa[kq + 2][row] = v.z; sa[kq + 3][row] = v.w;
        }
        if (NT) {
            const int row = tid >> 2, kq = (tid & 3) * 4;
            f32x4 v = f32x4{0, 0, 0, 0};
            if (n0 + row < N && k0 + kq < K) v = *(const f32x4*)(Bm + (long)(n0 + row) * ldb + k0 + kq);
            sb[kq + 0][row] = v.x; sb[kq + 1][row] = v.y; sb[kq + 2][row] = v.z; sb[kq + 3][row] = v.w;
        } else {
            const int kr = tid >> 4, cq = (tid & 15) * 4;
            f32x4 v = f32x4{0, 0, 0, 0};
            if (k0 + kr < K && n0 + cq < N) v = *(const f32x4*)(Bm + (long)(k0 + kr) * ldb + n0 + cq);
            *(f32x4*)&sb[kr][cq] = v;
        }
        __syncthreads();
        float step[4][4];      // the 16 products of a step are summed on their own and added once: an addition chain of 16 + K / 16, not K
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const f32x4 a = *(const f32x4*)&sa[kk][ty * 4], b = *(const f32x4*)&sb[kk][tx * 4];
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) step[r][c] = kk == 0 ? av[r] * bv[c] : fmaf(av[r], bv[c], step[r][c]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] += step[r][c];
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty * 4 + r, n = n0 + tx * 4;
        if (i < M && n < N) *(f32x4*)(C + (long)i * ldc + n) = f32x4{acc[r][0], acc[r][1], acc[r][2], acc[r][3]};      // (N is a multiple of 4)
    }
}

// 256 values in thread order -> their sum in a fixed tree, on every thread
__device__ __forceinline__ float block_sum(float v, float* s_red) {
    const int tid = threadIdx.x;
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    return s_red[0];
}

// (value, index) pairs -> the smallest value and, among equals, the lowest index; on every thread.  i < 0: no candidate.
__device__ __forceinline__ void block_argmin(float& v, int& i, float* s_rv, int* s_ri) {
    const int tid = threadIdx.x;
    __syncthreads();
    s_rv[tid] = v; s_ri[tid] = i;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float ov = s_rv[tid + o];
            const int oi = s_ri[tid + o], mi = s_ri[tid];
            if (oi >= 0 && (mi < 0 || ov < s_rv[tid] || (ov == s_rv[tid] && oi < mi))) { s_rv[tid] = ov; s_ri[tid] = oi; }
        }
        __syncthreads();
    }
    v = s_rv[0]; i = s_ri[0];
}

__device__ __forceinline__ float sign_f(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

struct TpMargin { int kind; int m_int; float m, cos_m, sin_m, thresh; };

// the positive side's transform f(S) of loss.py:537-560 and its derivative (tf.sign and the branch choices carry no gradient);
// arc margin: 1 - S^2 is clamped at 1e-12 in the derivative only, so it is finite at |S| = 1
__device__ __forceinline__ void tp_positive(const TpMargin& mg, float s, float& f, float& df) {
    if (mg.kind == XV_LOSS_ASOFTMAX) {
        if (mg.m_int == 1) { f = s; df = 1.f; }
        else if (mg.m_int == 2) { const float sg = sign_f(s); f = 2.f * (sg * (s * s)) - 1.f; df = 4.f * sg * s; }
        else {
            const float c2 = s * s, c4 = c2 * c2, s0 = sign_f(s), s3 = sign_f(2.f * c2 - 1.f) * s0, s4 = 2.f * s0 + s3 - 3.f;
            f = s3 * (8.f * c4 - 8.f * c2 + 1.f) + s4;
            df = s3 * (32.f * c2 * s - 16.f * s);
        }
    } else if (mg.kind == XV_LOSS_AMSOFTMAX) {
        f = s - mg.m; df = 1.f;
    } else {
        const float q = 1.f - s * s;
        const float nf = s * mg.cos_m - sqrtf(fmaxf(q, 0.f)) * mg.sin_m;
        const float nd = mg.cos_m + s / sqrtf(fmaxf(q, TP_EPS)) * mg.sin_m;
        if (s <= mg.thresh) { f = -nf - 2.f; df = -nd; } else { f = nf; df = nd; }
    }
}

// One workgroup per anchor row x.  dp[x][j] = d (sum of the loss terms) / d (pair matrix entry before clip / max), part[x] = {sum,
// valid count, positive count, 0}.  Columns B .. bp of dp are zeroed.
template <int KIND>
__global__ __launch_bounds__(256) void pair_rows_kernel(const float* __restrict__ G, int B, int bp, const int* __restrict__ labels, int squared,
                                                        float margin, TpMargin mg, float* __restrict__ dp, float* __restrict__ part) {
    XV_EW_PRIORITY();
    __shared__ float s_v[TP_MAX_B], s_f[TP_MAX_B], s_rv[256];
    __shared__ int s_lab[TP_MAX_B], s_sel[TP_MAX_B], s_pos[TP_MAX_B], s_ri[256], s_npos;
    const int tid = threadIdx.x, x = blockIdx.x;
    const float gxx = G[(long)x * bp + x];
    const int labx = labels[x];
    float chain[TP_Q], own[TP_Q], dfv[TP_Q];      // d value / d raw entry; this thread's own gradient count; f'(S)
    float rx = 0.f;
    if (KIND != TP_SEMIHARD) rx = 1.f / sqrtf(fmaxf(gxx, TP_EPS));
#pragma unroll
    for (int q = 0; q < TP_Q; ++q) {
        const int j = tid + 256 * q;
        chain[q] = own[q] = dfv[q] = 0.f;
        if (j >= B) continue;
        const float g = G[(long)x * bp + j], gjj = G[(long)j * bp + j];
        s_lab[j] = labels[j];
        s_sel[j] = -1;
        if (KIND == TP_SEMIHARD) {
            const float raw = (gxx - 2.f * g) + gjj, d2 = fmaxf(raw, 0.f), pass = raw >= 0.f ? 1.f : 0.f;
            if (squared) { s_v[j] = d2; chain[q] = pass; }
            else {
                const float d = d2 == 0.f ? 0.f : sqrtf(d2);
                s_v[j] = d;
                chain[q] = d2 == 0.f ? 0.f : pass * (0.5f / d);
            }
        } else {
            const float u = g * (rx * (1.f / sqrtf(fmaxf(gjj, TP_EPS))));
            const float s = fminf(fmaxf(u, -1.f), 1.f);
            chain[q] = (u >= -1.f && u <= 1.f) ? 1.f : 0.f;
            float f, df;
            tp_positive(mg, s, f, df);
            s_v[j] = s; s_f[j] = f; dfv[q] = df;
        }
    }
    __syncthreads();
    // the anchor's positives in ascending order (wave 0: a ballot per 64 columns): a scan over them does not filter all B columns
    if (KIND != TP_HARD && tid < 64) {
        int count = 0;
        for (int base = 0; base < B; base += 64) {
            const int j = base + tid;
            const bool is_pos = j < B && j != x && s_lab[j] == labx;
            const unsigned long long m = __ballot(is_pos);
            if (is_pos) s_pos[count + __popcll(m & ((1ull << tid) - 1ull))] = j;
            count += __popcll(m);
        }
        if (tid == 0) s_npos = count;
    }
    __syncthreads();
    const int npos = KIND != TP_HARD ? s_npos : 0;
    float sum = 0.f, n_valid = 0.f, n_pos = 0.f;
    if (KIND == TP_SEMIHARD) {
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= B || j == x || s_lab[j] != labx) continue;
            const float dxi = s_v[j];
            float vmin = 0.f, vout = 0.f, vin = 0.f;
            int imin = -1, iout = -1, iin = -1;
            for (int y = 0; y < B; ++y) {
                const float d = s_v[y];
                if (imin < 0 || d < vmin) { vmin = d; imin = y; }
                if (s_lab[y] == labx) continue;
                if (iin < 0 || d > vin) { vin = d; iin = y; }
                if (d > dxi && (iout < 0 || d < vout)) { vout = d; iout = y; }
            }
            const float negv = iout >= 0 ? vout : (iin >= 0 ? vin : vmin);
            const int negi = iout >= 0 ? iout : (iin >= 0 ? iin : imin);
            const float t = margin + (dxi - negv);
            n_valid += 1.f;
            if (t >= 0.f) { sum += t; own[q] = 1.f; s_sel[j] = negi; }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= bp) continue;
            float cnt = 0.f;
            if (j < B)
                for (int p = 0; p < npos; ++p) cnt += s_sel[s_pos[p]] == j ? 1.f : 0.f;      // (only a positive column has chosen a negative)
            dp[(long)x * bp + j] = j < B ? (own[q] - cnt) * chain[q] : 0.f;
        }
    } else if (KIND == TP_ALL) {
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= bp) continue;
            float grad = 0.f;
            if (j < B && j != x) {
                if (s_lab[j] != labx) {      // j is a negative: every positive k
                    const float sn = s_v[j];
                    float c = 0.f;
                    for (int p = 0; p < npos; ++p) {
                        const float t = sn - s_f[s_pos[p]];
                        n_valid += 1.f;
                        if (t >= 0.f) { sum += t; c += 1.f; }
                        if (t > TP_EPS) n_pos += 1.f;
                    }
                    grad = c;
                } else {                      // j is a positive: every negative k
                    const float fp = s_f[j];
                    float c = 0.f;
                    for (int k = 0; k < B; ++k) c += (s_lab[k] != labx && s_v[k] - fp >= 0.f) ? 1.f : 0.f;
                    grad = -c * dfv[q];
                }
            }
            dp[(long)x * bp + j] = j < B ? grad * chain[q] : 0.f;
        }
    } else {
        // the hardest positive and negative with the fillers of loss.py:617-625: the row maximum of f(S) where there is no positive, the row
        // MINIMUM OF f(S) (not of S) where there is no negative
        float vmax = 0.f, vmin = 0.f;
        int imax = -1, imin = -1;
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= B) continue;
            const float f = s_f[j];
            if (imax < 0 || -f < vmax) { vmax = -f; imax = j; }
            if (imin < 0 || f < vmin) { vmin = f; imin = j; }
        }
        block_argmin(vmax, imax, s_rv, s_ri);
        block_argmin(vmin, imin, s_rv, s_ri);
        const float fmax_row = -vmax, fmin_row = vmin;
        float vp = 0.f, vn = 0.f;
        int ip = -1, in = -1;
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= B) continue;
            const bool same = s_lab[j] == labx;
            const float ap = (same && j != x) ? s_f[j] : fmax_row;
            const float an = same ? fmin_row : s_v[j];
            if (ip < 0 || ap < vp) { vp = ap; ip = j; }
            if (in < 0 || -an < vn) { vn = -an; in = j; }
        }
        block_argmin(vp, ip, s_rv, s_ri);
        block_argmin(vn, in, s_rv, s_ri);
        const float hp = vp, hn = -vn, t = hn - hp;
        const bool p_real = s_lab[ip] == labx && ip != x, n_real = s_lab[in] != labx;
        const int jp = p_real ? ip : imax, jn = n_real ? in : imin;      // where the two gradients land
        const float w = t >= 0.f ? 1.f : 0.f;
        if (tid == 0) { sum = fmaxf(t, 0.f); n_valid = 1.f; n_pos = t > 0.f ? 1.f : 0.f; }
#pragma unroll
        for (int q = 0; q < TP_Q; ++q) {
            const int j = tid + 256 * q;
            if (j >= bp) continue;
            float grad = 0.f;
            if (j < B) {
                if (j == jp) grad -= w * dfv[q];
                if (j == jn) grad += n_real ? w : w * dfv[q];
            }
            dp[(long)x * bp + j] = j < B ? grad * chain[q] : 0.f;
        }
    }
    sum = block_sum(sum, s_rv);
    n_valid = block_sum(n_valid, s_rv);
    n_pos = block_sum(n_pos, s_rv);
    if (tid == 0) *(f32x4*)(part + 4 * (long)x) = f32x4{sum, n_valid, n_pos, 0.f};
}

// part[B][4] in index order (double accumulators: a count above 2^24 stays exact) -> loss, stats {valid, positive, fraction, 0}, scal[0] = 1 / normaliser
__global__ __launch_bounds__(256) void pair_finish_kernel(const float* __restrict__ part, int B, int kind, float* __restrict__ loss,
                                                          float* __restrict__ stats, float* __restrict__ scal) {
    __shared__ double s_d[3][256];
    const int tid = threadIdx.x;
    double a[3] = {0, 0, 0};
    for (int r = tid; r < B; r += 256)
        for (int c = 0; c < 3; ++c) a[c] += (double)part[4 * (long)r + c];
    for (int c = 0; c < 3; ++c) s_d[c][tid] = a[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int c = 0; c < 3; ++c) s_d[c][tid] += s_d[c][tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    const double sum = s_d[0][0], valid = s_d[1][0], pos = s_d[2][0];
    double den, frac;
    if (kind == TP_SEMIHARD) { den = valid > 1e-16 ? valid : 1e-16; frac = 0.0; }
    else if (kind == TP_ALL) { den = pos + 1e-16; frac = pos / (valid + 1e-16); }
    else { den = (double)B; frac = pos / (double)B; }
    const float inv = (float)(1.0 / den);
    *loss = (float)(sum / den);
    if (stats) { stats[0] = (float)valid; stats[1] = kind == TP_SEMIHARD ? 0.f : (float)pos; stats[2] = (float)frac; stats[3] = 0.f; }
    scal[0] = inv;
}

// A[i][:] = scale * (dG + dG^T)[i][:] for the whole pitch (columns B .. bp: 0), one workgroup per row.
//   cosine:    dG_ij = dp_ij r_i r_j; the chain through r_i (r = rsqrt(max(G_ii, 1e-12)), 0 where clamped) is -r_i^2 sum_j A_ij G_ij on the diagonal
//   Euclidean: dG_ij = -2 dp_ij, dG_ii += dp_ij, dG_jj += dp_ij
__global__ __launch_bounds__(256) void pair_sym_kernel(const float* __restrict__ G, const float* __restrict__ dp, int B, int bp, int cosine,
                                                       const float* __restrict__ scal, float* __restrict__ A) {
    XV_EW_PRIORITY();
    __shared__ float s_red[256];
    const int tid = threadIdx.x, i = blockIdx.x;
    const float scale = scal[0], gii = G[(long)i * bp + i];
    const float ri = cosine ? 1.f / sqrtf(fmaxf(gii, TP_EPS)) : 0.f;
    float acc = 0.f, diag = 0.f;
#pragma unroll
    for (int q = 0; q < TP_Q; ++q) {
        const int j = tid + 256 * q;
        if (j >= bp) continue;
        float a = 0.f;
        if (j < B) {
            const float p = dp[(long)i * bp + j] + dp[(long)j * bp + i];
            if (cosine) {
                const float rj = 1.f / sqrtf(fmaxf(G[(long)j * bp + j], TP_EPS));
                a = scale * p * (ri * rj);
                acc += a * G[(long)i * bp + j];
            } else {
                a = -2.f * scale * p;
                acc += p;
            }
            if (j == i) diag = cosine ? a : dp[(long)i * bp + i];
        }
        if (j != i) A[(long)i * bp + j] = a;
    }
    acc = block_sum(acc, s_red);
    if ((i & 255) == tid) {
        if (cosine) A[(long)i * bp + i] = diag + (gii >= TP_EPS ? -(ri * ri) * acc : 0.f);
        else A[(long)i * bp + i] = 2.f * scale * (acc - 2.f * diag);
    }
}

// ---- end-to-end validation loss (loss.py:666-702) from G: with u_ij = G_ij r_i r_j the cosine of rows i and j,
//   |sum of speaker s|^2 = sum_{m, m' in s} u_mm',   x_i . (sum of s) = sum_{m in s} u_im,   and the same sums without row i for i's own speaker
// one wave per speaker: nrm[s] = |speaker sum|^2
__global__ __launch_bounds__(64) void e2e_speaker_kernel(const float* __restrict__ G, int bp, int M, float* __restrict__ nrm) {
    const int s = blockIdx.x, lane = threadIdx.x, r0 = s * M;
    float acc = 0.f;
    for (int p = lane; p < M * M; p += 64) {
        const int a = r0 + p / M, b = r0 + p % M;
        const float ra = 1.f / sqrtf(fmaxf(G[(long)a * bp + a], TP_EPS)), rb = 1.f / sqrtf(fmaxf(G[(long)b * bp + b], TP_EPS));
        acc += G[(long)a * bp + b] * (ra * rb);
    }
    acc = wave_sum(acc);
    if (lane == 0) nrm[s] = acc;
}

// one workgroup per row: logits over the N speakers (x 20), the row's sparse softmax cross-entropy
__global__ __launch_bounds__(256) void e2e_rows_kernel(const float* __restrict__ G, int bp, int N, int M, const float* __restrict__ nrm,
                                                       float* __restrict__ row_loss) {
    XV_EW_PRIORITY();
    __shared__ float s_u[TP_MAX_B], s_logit[TP_MAX_B], s_red[256];
    __shared__ int s_ri[256];
    const int tid = threadIdx.x, i = blockIdx.x, B = N * M, own = i / M;
    const float ri = 1.f / sqrtf(fmaxf(G[(long)i * bp + i], TP_EPS));
    for (int j = tid; j < B; j += 256) s_u[j] = G[(long)i * bp + j] * (ri * (1.f / sqrtf(fmaxf(G[(long)j * bp + j], TP_EPS))));
    // |own speaker's sum without row i|^2, from the pairs of the own block that do not touch i
    float ex = 0.f;
    for (int p = tid; p < M * M; p += 256) {
        const int a = own * M + p / M, b = own * M + p % M;
        if (a == i || b == i) continue;
        const float ra = 1.f / sqrtf(fmaxf(G[(long)a * bp + a], TP_EPS)), rb = 1.f / sqrtf(fmaxf(G[(long)b * bp + b], TP_EPS));
        ex += G[(long)a * bp + b] * (ra * rb);
    }
    ex = block_sum(ex, s_red);
    for (int s = tid; s < N; s += 256) {
        float dot = 0.f;
        for (int m = 0; m < M; ++m) {
            const int j = s * M + m;
            if (j != i) dot += s_u[j];      // (row i itself belongs to its own speaker only)
        }
        float sim;
        if (s == own) sim = dot / sqrtf(fmaxf(ex, TP_EPS));                       // the exclusive sum, normalised (no 1 / (M - 1): loss.py:677)
        else { const float mf = (float)M; sim = (dot / mf) / sqrtf(fmaxf(nrm[s] / (mf * mf), TP_EPS)); }
        s_logit[s] = 20.f * sim;
    }
    __syncthreads();
    float mx = -INFINITY;
    int mi = -1;
    for (int s = tid; s < N; s += 256)
        if (mi < 0 || -s_logit[s] < mx) { mx = -s_logit[s]; mi = s; }
    block_argmin(mx, mi, s_red, s_ri);
    const float top = -mx;
    float z = 0.f;
    for (int s = tid; s < N; s += 256) z += expf(s_logit[s] - top);
    z = block_sum(z, s_red);
    if (tid == 0) row_loss[i] = (logf(z) + top) - s_logit[own];
}

__global__ __launch_bounds__(256) void e2e_finish_kernel(const float* __restrict__ row_loss, int B, float* __restrict__ loss) {
    __shared__ float s_red[256];
    float a = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) a += row_loss[r];
    a = block_sum(a, s_red);
    if (threadIdx.x == 0) *loss = a / (float)B;
}

struct TpPlan { int kind; int cosine; TpMargin mg; };

static int tp_check(const char* who, const xv_pair_loss_config* cfg, const float* x, int b, int d, int ldx, const void* ws, size_t ws_bytes,
                    TpPlan* p) {
    XV_REQUIRE(cfg, "%s: null xv_pair_loss_config", who);
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_pair_loss_config),
               "%s: xv_pair_loss_config.struct_bytes is %d, this library's struct has %zu bytes", who, cfg->struct_bytes, sizeof(xv_pair_loss_config));
    XV_REQUIRE(cfg->kind == XV_PAIR_SEMIHARD || cfg->kind == XV_PAIR_ANGULAR, "%s: pair loss kind %d is neither semi-hard (0) nor angular (1)", who,
               cfg->kind);
    XV_REQUIRE(b >= 1 && b <= TP_MAX_B, "%s: %d rows, 1 .. %d are supported", who, b, TP_MAX_B);
    XV_REQUIRE(d >= 4 && d % 4 == 0, "%s: the embedding dimension %d must be a positive multiple of 4", who, d);
    XV_REQUIRE(ldx >= d && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "%s: x needs 16-byte aligned rows (pitch %d, dimension %d)", who, ldx, d);
    XV_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= tp_layout(b).total * sizeof(float),
               "%s: the workspace needs %zu bytes (xv_pair_loss_workspace_bytes), 16-byte aligned; %zu given", who, tp_layout(b).total * sizeof(float),
               ws_bytes);
    memset(p, 0, sizeof(*p));
    if (cfg->kind == XV_PAIR_SEMIHARD) { p->kind = TP_SEMIHARD; return 0; }
    XV_REQUIRE(cfg->triplet_type == XV_TRIPLET_ALL || cfg->triplet_type == XV_TRIPLET_HARD, "%s: triplet_type %d is neither all (0) nor hard (1)", who,
               cfg->triplet_type);
    XV_REQUIRE(cfg->margin_kind >= XV_LOSS_ASOFTMAX && cfg->margin_kind <= XV_LOSS_ARCSOFTMAX,
               "%s: margin_kind %d is not asoftmax (1), additive_margin_softmax (2) or additive_angular_margin_softmax (3)", who, cfg->margin_kind);
    p->kind = cfg->triplet_type == XV_TRIPLET_ALL ? TP_ALL : TP_HARD;
    p->cosine = 1;
    p->mg.kind = cfg->margin_kind;
    p->mg.m = cfg->margin;
    p->mg.m_int = (int)cfg->margin;
    if (cfg->margin_kind == XV_LOSS_ASOFTMAX)
        XV_REQUIRE(p->mg.m_int == 1 || p->mg.m_int == 2 || p->mg.m_int == 4, "%s: [ERROR] m=%d is not unsupported if asoftmax is selected.", who, p->mg.m_int);
    const double m = (double)cfg->margin, pi = 3.14159265358979323846;
    p->mg.cos_m = (float)cos(m); p->mg.sin_m = (float)sin(m); p->mg.thresh = (float)cos(pi - m);
    return 0;
}

static int tp_gram(hipStream_t s, const float* x, int b, int d, int ldx, float* g, int bp) {
    pair_gemm_kernel<true><<<dim3(xv_cdiv(b, 64), xv_cdiv(b, 64)), 256, 0, s>>>(x, ldx, x, ldx, b, b, d, g, bp);      // (columns B .. bp of G: 0)
    XV_LAUNCH_CHECK();
    return 0;
}


// ---- GE2E training loss (loss.py:903-982; include/xvector_hip.h "GE2E training loss") from the same u_ij = G_ij r_i r_j:
//   t_ik = sum_{m in k} u_im = x^_i . (sum of speaker k),   n_k = sum_{m, m' in k} u_mm' = |sum of speaker k|^2 (e2e_speaker_kernel),
//   c_ik = t_ik / sqrt(max(n_k, 1e-12)) for another speaker's k; for the own speaker both sums run over the pairs that do not touch row i
//   ge2e_rows_kernel<TYPE>   one workgroup per row: c and P = d (sum of the row losses) / d S for the N speakers, the row's (loss, sum P c, sum P)
//   ge2e_finish_kernel       the B partials in index order in double -> loss, d w, d b; scal = {1 / B, d w, d b}
//   ge2e_q_kernel            Q = d (sum of the row losses) / d u [B x B] from P, c and the norms -> pair_sym_kernel -> pair_gemm_kernel<false>
enum { GE_SOFTMAX = 0, GE_CONTRASTIVE = 1 };
#define GE_MAX_N (TP_MAX_B / 2)      // at least two segments per speaker

struct GeLayout { size_t nrm, p, c, ex, total; int np; };
static GeLayout ge_layout(int n, int m) {
    const TpLayout t = tp_layout(n * m);
    GeLayout l;
    l.np = (n + 3) / 4 * 4;
    const size_t bn = (size_t)n * m * l.np;
    l.nrm = t.total; l.p = l.nrm + l.np; l.c = l.p + bn; l.ex = l.c + bn; l.total = l.ex + t.bp;
    return l;
}

// 1 / (1 + exp(-s)) without a difference of nearly equal numbers on either side: sigmoid(-s) is 1 - sigmoid(s) to its own rounding
__device__ __forceinline__ float sigmoid_f(float s) {
    const float e = expf(-fabsf(s)), hi = 1.f / (1.f + e);
    return s >= 0.f ? hi : e * hi;
}

// One workgroup per row i.  cmat[i][k] = c_ik, pmat[i][k] = P_ik WITHOUT the 1 / B of the mean, exn[i] = the own speaker's exclusive norm,
// part[i] = {row loss, sum_k P_ik c_ik, sum_k P_ik, 0}.  The contrastive maximum is taken where S is largest (the sigmoid is monotone and
// saturates in fp32 long before S does); a tie goes to the lowest index.
template <int TYPE>
__global__ __launch_bounds__(256) void ge2e_rows_kernel(const float* __restrict__ G, int bp, int N, int M, const float* __restrict__ nrm,
                                                        const float* __restrict__ wp, const float* __restrict__ bptr, int np,
                                                        float* __restrict__ pmat, float* __restrict__ cmat, float* __restrict__ exn,
                                                        float* __restrict__ part) {
    XV_EW_PRIORITY();
    __shared__ float s_u[TP_MAX_B], s_logit[GE_MAX_N], s_c[GE_MAX_N], s_red[256];
    __shared__ int s_ri[256];
    const int tid = threadIdx.x, i = blockIdx.x, B = N * M, own = i / M;
    const float aw = fabsf(wp[0]), off = bptr[0];
    const float ri = 1.f / sqrtf(fmaxf(G[(long)i * bp + i], TP_EPS));
    for (int j = tid; j < B; j += 256) s_u[j] = G[(long)i * bp + j] * (ri * (1.f / sqrtf(fmaxf(G[(long)j * bp + j], TP_EPS))));
    float ex = 0.f;      // |own speaker's sum without row i|^2, from the pairs of the own block that do not touch i
    for (int p = tid; p < M * M; p += 256) {
        const int a = own * M + p / M, b = own * M + p % M;
        if (a == i || b == i) continue;
        const float ra = 1.f / sqrtf(fmaxf(G[(long)a * bp + a], TP_EPS)), rb = 1.f / sqrtf(fmaxf(G[(long)b * bp + b], TP_EPS));
        ex += G[(long)a * bp + b] * (ra * rb);
    }
    ex = block_sum(ex, s_red);
    for (int s = tid; s < N; s += 256) {
        float dot = 0.f;
        for (int m = 0; m < M; ++m) {
            const int j = s * M + m;
            if (j != i) dot += s_u[j];
        }
        const float c = dot * (1.f / sqrtf(fmaxf(s == own ? ex : nrm[s], TP_EPS)));
        s_c[s] = c;
        s_logit[s] = aw * c + off;
    }
    __syncthreads();
    float row = 0.f, pc = 0.f, ps = 0.f;
    if (TYPE == GE_SOFTMAX) {
        float mx = 0.f;
        int mi = -1;
        for (int s = tid; s < N; s += 256)
            if (mi < 0 || -s_logit[s] < mx) { mx = -s_logit[s]; mi = s; }
        block_argmin(mx, mi, s_red, s_ri);
        const float top = -mx;
        float z = 0.f;
        for (int s = tid; s < N; s += 256) z += expf(s_logit[s] - top);
        z = block_sum(z, s_red);
        for (int s = tid; s < N; s += 256) {
            const float p = expf(s_logit[s] - top) / z - (s == own ? 1.f : 0.f);
            pmat[(long)i * np + s] = p; cmat[(long)i * np + s] = s_c[s];
            pc += p * s_c[s]; ps += p;
        }
        row = (logf(z) + top) - s_logit[own];
    } else {
        float mx = 0.f;
        int mi = -1;
        for (int s = tid; s < N; s += 256)
            if (s != own && (mi < 0 || -s_logit[s] < mx)) { mx = -s_logit[s]; mi = s; }
        block_argmin(mx, mi, s_red, s_ri);
        for (int s = tid; s < N; s += 256) {
            const float sg = s_logit[s], d = sigmoid_f(sg) * sigmoid_f(-sg);
            const float p = s == own ? -d : (s == mi ? d : 0.f);
            pmat[(long)i * np + s] = p; cmat[(long)i * np + s] = s_c[s];
            pc += p * s_c[s]; ps += p;
        }
        row = sigmoid_f(-s_logit[own]) + (mi >= 0 ? sigmoid_f(s_logit[mi]) : 0.f);      // (one speaker: the masked 0 is the maximum)
    }
    pc = block_sum(pc, s_red);
    ps = block_sum(ps, s_red);
    if (tid == 0) {
        *(f32x4*)(part + 4 * (long)i) = f32x4{row, pc, ps, 0.f};
        exn[i] = ex;
    }
}

// part[B][4] in index order in double -> loss (the mean), stats {d w, d b, 0, 0}, scal = {1 / B, d w = sign(w) sum P c / B, d b = sum P / B}
__global__ __launch_bounds__(256) void ge2e_finish_kernel(const float* __restrict__ part, int B, const float* __restrict__ wp, float* __restrict__ loss,
                                                          float* __restrict__ stats, float* __restrict__ scal) {
    __shared__ double s_d[3][256];
    const int tid = threadIdx.x;
    double a[3] = {0, 0, 0};
    for (int r = tid; r < B; r += 256)
        for (int c = 0; c < 3; ++c) a[c] += (double)part[4 * (long)r + c];
    for (int c = 0; c < 3; ++c) s_d[c][tid] = a[c];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o)
            for (int c = 0; c < 3; ++c) s_d[c][tid] += s_d[c][tid + o];
        __syncthreads();
    }
    if (tid != 0) return;
    const double den = (double)B;
    const float dw = (float)((double)sign_f(wp[0]) * (s_d[1][0] / den)), db = (float)(s_d[2][0] / den);
    *loss = (float)(s_d[0][0] / den);
    if (stats) { stats[0] = dw; stats[1] = db; stats[2] = 0.f; stats[3] = 0.f; }
    scal[0] = (float)(1.0 / den); scal[1] = dw; scal[2] = db;
}

// One workgroup per row a of Q = d (sum of the row losses) / d u, every entry of u taken as a variable of its own (pair_sym_kernel adds Q^T).
//   j in another speaker k:   |w| P_ak / sqrt(max(n_k, eps))                                                   (t_ak)
//   j in the own speaker k:   -1/2 |w| / n_k sum_{i not in k} P_ik c_ik                                        (n_k; 0 where clamped)
//                             + sum_{i in k, i != a, i != j} -1/2 |w| / ex_i P_ik c_ik, in index order         (ex_i; 0 where clamped)
//                             + (j != a) |w| P_ak / sqrt(max(ex_a, eps))                                       (the exclusive t_a)
// (t n^-3/2 = c / n).  Columns B .. bp are zeroed.
__global__ __launch_bounds__(256) void ge2e_q_kernel(int N, int M, int bp, int np, const float* __restrict__ nrm, const float* __restrict__ pmat,
                                                     const float* __restrict__ cmat, const float* __restrict__ exn, const float* __restrict__ wp,
                                                     float* __restrict__ dp) {
    XV_EW_PRIORITY();
    __shared__ float s_de[TP_MAX_B], s_red[256];
    const int tid = threadIdx.x, a = blockIdx.x, B = N * M, ka = a / M, r0 = ka * M;
    const float aw = fabsf(wp[0]);
    float v = 0.f;
    for (int i = tid; i < B; i += 256)
        if (i / M != ka) v += pmat[(long)i * np + ka] * cmat[(long)i * np + ka];
    v = block_sum(v, s_red);
    const float nk = nrm[ka];
    const float dn = nk >= TP_EPS ? (-0.5f * aw) * (v / nk) : 0.f;
    for (int m = tid; m < M; m += 256) {
        const int i = r0 + m;
        const float e = exn[i];
        s_de[m] = e >= TP_EPS ? (-0.5f * aw) * ((pmat[(long)i * np + ka] * cmat[(long)i * np + ka]) / e) : 0.f;
    }
    __syncthreads();
    const float own_t = aw * pmat[(long)a * np + ka] * (1.f / sqrtf(fmaxf(exn[a], TP_EPS)));
#pragma unroll
    for (int q = 0; q < TP_Q; ++q) {
        const int j = tid + 256 * q;
        if (j >= bp) continue;
        float qv = 0.f;
        if (j < B) {
            const int k = j / M;
            if (k != ka) qv = aw * pmat[(long)a * np + k] * (1.f / sqrtf(fmaxf(nrm[k], TP_EPS)));
            else {
                qv = dn;
                for (int m = 0; m < M; ++m)
                    if (r0 + m != a && r0 + m != j) qv += s_de[m];
                if (j != a) qv += own_t;
            }
        }
        dp[(long)a * bp + j] = qv;
    }
}

static int ge_check(const char* who, const xv_ge2e_config* cfg, const float* x, int d, int ldx, const float* w, const float* b, const void* ws,
                    size_t ws_bytes) {
    XV_REQUIRE(cfg, "%s: null xv_ge2e_config", who);
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_ge2e_config), "%s: xv_ge2e_config.struct_bytes is %d, this library's struct has %zu bytes", who,
               cfg->struct_bytes, sizeof(xv_ge2e_config));
    XV_REQUIRE(cfg->loss_type == XV_GE2E_SOFTMAX || cfg->loss_type == XV_GE2E_CONTRASTIVE, "%s: The GE2E only support softmax and contrastive loss (loss_type %d)",
               who, cfg->loss_type);
    XV_REQUIRE(cfg->speakers >= 1 && cfg->segments >= 1, "%s: %d speakers x %d segments", who, cfg->speakers, cfg->segments);
    XV_REQUIRE(cfg->segments != 1, "%s: num_segments_per_speaker is 1: a row needs another row of its speaker (assert num_segments_per_speaker != 1)", who);
    XV_REQUIRE((long)cfg->speakers * cfg->segments <= TP_MAX_B, "%s: %d speakers x %d segments, 1 .. %d rows are supported", who, cfg->speakers,
               cfg->segments, TP_MAX_B);
    XV_REQUIRE(d >= 4 && d % 4 == 0, "%s: the embedding dimension %d must be a positive multiple of 4", who, d);
    XV_REQUIRE(ldx >= d && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "%s: x needs 16-byte aligned rows (pitch %d, dimension %d)", who, ldx, d);
    XV_REQUIRE(w && b, "%s: w and b (one device float each) must be given", who);
    const size_t need = ge_layout(cfg->speakers, cfg->segments).total * sizeof(float);
    XV_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need, "%s: the workspace needs %zu bytes (xv_ge2e_loss_workspace_bytes), 16-byte aligned; %zu given",
               who, need, ws_bytes);
    return 0;
}

}  // namespace

extern "C" size_t xv_pair_loss_workspace_bytes(int b, int d) {
    if (b < 1 || b > TP_MAX_B) {
        xv_set_error("pair_loss_workspace_bytes: %d rows, 1 .. %d are supported", b, TP_MAX_B);
        return 0;
    }
    if (d < 4 || d % 4) {
        xv_set_error("pair_loss_workspace_bytes: the embedding dimension %d must be a positive multiple of 4", d);
        return 0;
    }
    return tp_layout(b).total * sizeof(float);
}

extern "C" int xv_pair_loss_forward(void* stream, const xv_pair_loss_config* cfg, const float* x, int b, int d, int ldx, const int32_t* labels,
                                    float* loss, float* stats, void* ws, size_t ws_bytes) {
    TpPlan p;
    int rc = tp_check("pair_loss_forward", cfg, x, b, d, ldx, ws, ws_bytes, &p);
    if (rc) return rc;
    XV_REQUIRE(labels && loss, "pair_loss_forward: labels and loss must be given");
    hipStream_t s = (hipStream_t)stream;
    const TpLayout l = tp_layout(b);
    float* w = (float*)ws;
    rc = tp_gram(s, x, b, d, ldx, w + l.g, l.bp);
    if (rc) return rc;
    if (p.kind == TP_SEMIHARD)
        pair_rows_kernel<TP_SEMIHARD><<<b, 256, 0, s>>>(w + l.g, b, l.bp, labels, cfg->squared != 0, cfg->margin, p.mg, w + l.dp, w + l.part);
    else if (p.kind == TP_ALL)
        pair_rows_kernel<TP_ALL><<<b, 256, 0, s>>>(w + l.g, b, l.bp, labels, 0, 0.f, p.mg, w + l.dp, w + l.part);
    else
        pair_rows_kernel<TP_HARD><<<b, 256, 0, s>>>(w + l.g, b, l.bp, labels, 0, 0.f, p.mg, w + l.dp, w + l.part);
    XV_LAUNCH_CHECK();
    pair_finish_kernel<<<1, 256, 0, s>>>(w + l.part, b, p.kind, loss, stats, w + l.scal);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_pair_loss_backward(void* stream, const xv_pair_loss_config* cfg, const float* x, int b, int d, int ldx, const int32_t* labels,
                                     void* ws, size_t ws_bytes, float* dx, int lddx) {
    TpPlan p;
    int rc = tp_check("pair_loss_backward", cfg, x, b, d, ldx, ws, ws_bytes, &p);
    if (rc) return rc;
    (void)labels;      // the forward call left every decision in ws
    XV_REQUIRE(dx && lddx >= d && lddx % 4 == 0 && ((uintptr_t)dx & 15) == 0, "pair_loss_backward: dx needs 16-byte aligned rows (pitch %d, dimension %d)",
               lddx, d);
    hipStream_t s = (hipStream_t)stream;
    const TpLayout l = tp_layout(b);
    float* w = (float*)ws;
    pair_sym_kernel<<<b, 256, 0, s>>>(w + l.g, w + l.dp, b, l.bp, p.cosine, w + l.scal, w + l.a);
    XV_LAUNCH_CHECK();
    pair_gemm_kernel<false><<<dim3(xv_cdiv(d, 64), xv_cdiv(b, 64)), 256, 0, s>>>(w + l.a, l.bp, x, ldx, b, d, b, dx, lddx);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_e2e_valid_loss(void* stream, const float* x, int speakers, int segments, int d, int ldx, float* loss, void* ws, size_t ws_bytes) {
    XV_REQUIRE(speakers >= 1 && segments >= 1 && (long)speakers * segments <= TP_MAX_B, "e2e_valid_loss: %d speakers x %d segments, 1 .. %d rows are supported",
               speakers, segments, TP_MAX_B);
    const int b = speakers * segments;
    XV_REQUIRE(d >= 4 && d % 4 == 0, "e2e_valid_loss: the embedding dimension %d must be a positive multiple of 4", d);
    XV_REQUIRE(ldx >= d && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0, "e2e_valid_loss: x needs 16-byte aligned rows (pitch %d, dimension %d)", ldx, d);
    XV_REQUIRE(loss && ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= tp_layout(b).total * sizeof(float),
               "e2e_valid_loss: the workspace needs %zu bytes (xv_pair_loss_workspace_bytes), 16-byte aligned; %zu given", tp_layout(b).total * sizeof(float),
               ws_bytes);
    hipStream_t s = (hipStream_t)stream;
    const TpLayout l = tp_layout(b);
    float* w = (float*)ws;
    int rc = tp_gram(s, x, b, d, ldx, w + l.g, l.bp);
    if (rc) return rc;
    float* nrm = w + l.dp;                 // [speakers]
    float* row_loss = w + l.dp + l.bp;     // [b]
    e2e_speaker_kernel<<<speakers, 64, 0, s>>>(w + l.g, l.bp, segments, nrm);
    XV_LAUNCH_CHECK();
    e2e_rows_kernel<<<b, 256, 0, s>>>(w + l.g, l.bp, speakers, segments, nrm, row_loss);
    XV_LAUNCH_CHECK();
    e2e_finish_kernel<<<1, 256, 0, s>>>(row_loss, b, loss);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t xv_ge2e_loss_workspace_bytes(int speakers, int segments, int d) {
    if (speakers < 1 || segments < 2 || (long)speakers * segments > TP_MAX_B) {
        xv_set_error("ge2e_loss_workspace_bytes: %d speakers x %d segments; at least 2 segments per speaker and 2 .. %d rows are supported", speakers,
                     segments, TP_MAX_B);
        return 0;
    }
    if (d < 4 || d % 4) {
        xv_set_error("ge2e_loss_workspace_bytes: the embedding dimension %d must be a positive multiple of 4", d);
        return 0;
    }
    return ge_layout(speakers, segments).total * sizeof(float);
}

extern "C" int xv_ge2e_loss_forward(void* stream, const xv_ge2e_config* cfg, const float* x, int d, int ldx, const float* w, const float* b,
                                    float* loss, float* stats, void* ws, size_t ws_bytes) {
    int rc = ge_check("ge2e_loss_forward", cfg, x, d, ldx, w, b, ws, ws_bytes);
    if (rc) return rc;
    XV_REQUIRE(loss, "ge2e_loss_forward: loss must be given");
    hipStream_t s = (hipStream_t)stream;
    const int n = cfg->speakers, m = cfg->segments, rows = n * m;
    const TpLayout l = tp_layout(rows);
    const GeLayout g = ge_layout(n, m);
    float* f = (float*)ws;
    rc = tp_gram(s, x, rows, d, ldx, f + l.g, l.bp);
    if (rc) return rc;
    e2e_speaker_kernel<<<n, 64, 0, s>>>(f + l.g, l.bp, m, f + g.nrm);
    XV_LAUNCH_CHECK();
    if (cfg->loss_type == XV_GE2E_SOFTMAX)
        ge2e_rows_kernel<GE_SOFTMAX><<<rows, 256, 0, s>>>(f + l.g, l.bp, n, m, f + g.nrm, w, b, g.np, f + g.p, f + g.c, f + g.ex, f + l.part);
    else
        ge2e_rows_kernel<GE_CONTRASTIVE><<<rows, 256, 0, s>>>(f + l.g, l.bp, n, m, f + g.nrm, w, b, g.np, f + g.p, f + g.c, f + g.ex, f + l.part);
    XV_LAUNCH_CHECK();
    ge2e_finish_kernel<<<1, 256, 0, s>>>(f + l.part, rows, w, loss, stats, f + l.scal);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_ge2e_loss_backward(void* stream, const xv_ge2e_config* cfg, const float* x, int d, int ldx, const float* w, const float* b, void* ws,
                                     size_t ws_bytes, float* dx, int lddx, float* dw, float* db) {
    int rc = ge_check("ge2e_loss_backward", cfg, x, d, ldx, w, b, ws, ws_bytes);
    if (rc) return rc;
    XV_REQUIRE(dx && lddx >= d && lddx % 4 == 0 && ((uintptr_t)dx & 15) == 0, "ge2e_loss_backward: dx needs 16-byte aligned rows (pitch %d, dimension %d)",
               lddx, d);
    XV_REQUIRE(dw && db, "ge2e_loss_backward: dw and db (one device float each) must be given");
    hipStream_t s = (hipStream_t)stream;
    const int n = cfg->speakers, m = cfg->segments, rows = n * m;
    const TpLayout l = tp_layout(rows);
    const GeLayout g = ge_layout(n, m);
    float* f = (float*)ws;
    ge2e_q_kernel<<<rows, 256, 0, s>>>(n, m, l.bp, g.np, f + g.nrm, f + g.p, f + g.c, f + g.ex, w, f + l.dp);
    XV_LAUNCH_CHECK();
    pair_sym_kernel<<<rows, 256, 0, s>>>(f + l.g, f + l.dp, rows, l.bp, 1, f + l.scal, f + l.a);
    XV_LAUNCH_CHECK();
    pair_gemm_kernel<false><<<dim3(xv_cdiv(d, 64), xv_cdiv(rows, 64)), 256, 0, s>>>(f + l.a, l.bp, x, ldx, rows, d, rows, dx, lddx);
    XV_LAUNCH_CHECK();
    rc = xv_copy_2d(s, dw, 1, f + l.scal + 1, 1, 1, 1);
    if (rc) return rc;
    return xv_copy_2d(s, db, 1, f + l.scal + 2, 1, 1, 1);
}
