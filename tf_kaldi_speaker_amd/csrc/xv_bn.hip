// BatchNorm (+ activation) forward and the activation context: column statistics of the frame-level tensors, their finalisation,
// output range, inference scale and the apply pass; the one-launch forms (forward and backward) for segment-level tensors, and the bare
// activation kernels.  All tensors fp32 row-major with the channel axis contiguous, so threads always run along channels (16 B per lane
// where the pitch allows) and reductions over rows are per-thread serial + LDS combine in a fixed order.  The backward family of the
// frame-level tensors is in xv_bn_bwd.hip.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_bn.h"
#include "xv_gemm.h"      // XV_TILE_M: the rows behind one partial of a GEMM epilogue

// bn_part layout: [2][tiles][n] with tiles = ceil(rows / XV_TILE_M): sum, then centred sum of squares.
// block = 256 threads = 32 columns x 8 row lanes over one 128-row tile; two passes (sum/min/max, then
// squares centred on the tile mean) with fixed-order combines through LDS.  Output layout: xv_epilogue.h.
__global__ __launch_bounds__(256) void col_stats_kernel(const float* __restrict__ z, int rows, int n, long ldz,
                                                        float* __restrict__ part, int tiles) {
    XV_EW_PRIORITY();
    __shared__ float red[8][32], rmin[8][32], rmax[8][32];
    __shared__ float s_mean[32];
    const int cx = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cx;
    const int tile = blockIdx.y;
    const int r0 = tile * XV_TILE_M, r1 = min(rows, r0 + XV_TILE_M);
    const long plane = (long)tiles * n;
    float s = 0.f, mn = INFINITY, mx = -INFINITY;
    if (col < n)
        for (int r = r0 + rl; r < r1; r += 8) {
            float v = z[(long)r * ldz + col];
            s += v; mn = fminf(mn, v); mx = fmaxf(mx, v);
        }
    red[rl][cx] = s; rmin[rl][cx] = mn; rmax[rl][cx] = mx;
    __syncthreads();
    if (rl == 0) {
        float t = 0.f, a = INFINITY, b = -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) { t += red[k][cx]; a = fminf(a, rmin[k][cx]); b = fmaxf(b, rmax[k][cx]); }
        if (col < n) {
            part[(long)tile * n + col] = t;
            part[2 * plane + (long)tile * n + col] = a;
            part[3 * plane + (long)tile * n + col] = b;
        }
        s_mean[cx] = t / (float)(r1 - r0);
    }
    __syncthreads();
    const float mean = s_mean[cx];
    float q = 0.f;
    if (col < n)
        for (int r = r0 + rl; r < r1; r += 8) {
            float d = z[(long)r * ldz + col] - mean;
            q += d * d;
        }
    __syncthreads();
    red[rl][cx] = q;
    __syncthreads();
    if (rl == 0 && col < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][cx];
        part[plane + (long)tile * n + col] = t;
    }
}

// The same statistics for rows of whole float4s (n and ldz multiples of 4, 16-byte aligned): ONE pass over memory.  block = 256 threads =
// 32 column quads x 8 row lanes over one 128-row tile; a thread keeps its 16 rows x 4 columns in registers, so the squares centred on the
// tile mean come from registers instead of a second read, and a wave instruction covers two rows of 512 contiguous bytes (the scalar
// form above: 128 bytes per row, every element read twice - 0.24-0.30 of the HBM rate in round 2).  Same fixed-order combines.
__global__ __launch_bounds__(256) void col_stats4_kernel(const float* __restrict__ z, int rows, int n, long ldz, float* __restrict__ part,
                                                         int tiles) {
    XV_EW_PRIORITY();
    __shared__ f32x4 red[8][32], rmin[8][32], rmax[8][32];
    __shared__ f32x4 s_mean[32];
    const int cq = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int col = (blockIdx.x * 32 + cq) * 4;
    const int tile = blockIdx.y;
    const int r0 = tile * XV_TILE_M, r1 = min(rows, r0 + XV_TILE_M);
    const long plane = (long)tiles * n;
    const bool cv = col < n;
    f32x4 v[XV_TILE_M / 8];
    f32x4 s = {0, 0, 0, 0}, mn = {INFINITY, INFINITY, INFINITY, INFINITY}, mx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    // unconditional loads (row / column clamped), all sixteen in flight: a predicated load compiles to a branch + s_waitcnt vmcnt(0)
    const float* __restrict__ zc = z + (cv ? col : 0);
#pragma unroll
    for (int i = 0; i < XV_TILE_M / 8; ++i) v[i] = *(const f32x4*)(zc + (long)min(r0 + rl + 8 * i, r1 - 1) * ldz);
#pragma unroll
    for (int i = 0; i < XV_TILE_M / 8; ++i) {
        const bool ok = cv && r0 + rl + 8 * i < r1;
        const f32x4 x = v[i];
        s += ok ? x : f32x4{0, 0, 0, 0};
        mn.x = ok ? fminf(mn.x, x.x) : mn.x; mn.y = ok ? fminf(mn.y, x.y) : mn.y; mn.z = ok ? fminf(mn.z, x.z) : mn.z; mn.w = ok ? fminf(mn.w, x.w) : mn.w;
        mx.x = ok ? fmaxf(mx.x, x.x) : mx.x; mx.y = ok ? fmaxf(mx.y, x.y) : mx.y; mx.z = ok ? fmaxf(mx.z, x.z) : mx.z; mx.w = ok ? fmaxf(mx.w, x.w) : mx.w;
    }
    red[rl][cq] = s; rmin[rl][cq] = mn; rmax[rl][cq] = mx;
    __syncthreads();
    if (rl == 0) {
        f32x4 t = {0, 0, 0, 0}, a = rmin[0][cq], b = rmax[0][cq];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            t += red[k][cq];
            const f32x4 u = rmin[k][cq], w = rmax[k][cq];
            a.x = fminf(a.x, u.x); a.y = fminf(a.y, u.y); a.z = fminf(a.z, u.z); a.w = fminf(a.w, u.w);
            b.x = fmaxf(b.x, w.x); b.y = fmaxf(b.y, w.y); b.z = fmaxf(b.z, w.z); b.w = fmaxf(b.w, w.w);
        }
        if (cv) {
            *(f32x4*)(part + (long)tile * n + col) = t;
            *(f32x4*)(part + 2 * plane + (long)tile * n + col) = a;
            *(f32x4*)(part + 3 * plane + (long)tile * n + col) = b;
        }
        s_mean[cq] = t / (float)(r1 - r0);
    }
    __syncthreads();
    const f32x4 mean = s_mean[cq];
    f32x4 q = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < XV_TILE_M / 8; ++i)
        if (cv && r0 + rl + 8 * i < r1) {
            const f32x4 d = v[i] - mean;
            q += d * d;
        }
    __syncthreads();
    red[rl][cq] = q;
    __syncthreads();
    if (rl == 0 && cv) {
        f32x4 t = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][cq];
        *(f32x4*)(part + plane + (long)tile * n + col) = t;
    }
}

// The form xv_col_stats runs: 4 = col_stats4_kernel (rows of whole, 16-byte aligned float4s on both sides), 1 = col_stats_kernel.
static int col_stats_form(int n, int ldz, uintptr_t z, uintptr_t bn_part) {
    return (n % 4 == 0 && ldz % 4 == 0 && z % 16 == 0 && bn_part % 16 == 0) ? 4 : 1;
}
extern "C" int xv_debug_col_stats_form(int n, int ldz, uintptr_t z, uintptr_t bn_part) { return col_stats_form(n, ldz, z, bn_part); }

extern "C" int xv_col_stats(void* stream, const float* z, int rows, int n, int ldz, float* bn_part) {
    XV_REQUIRE(rows > 0 && n > 0 && ldz >= n, "col_stats: bad shape");
    int tiles = xv_cdiv(rows, XV_TILE_M);
    if (col_stats_form(n, ldz, (uintptr_t)z, (uintptr_t)bn_part) == 4)
        hipLaunchKernelGGL(col_stats4_kernel, dim3(xv_cdiv(n, 128), tiles), dim3(256), 0, (hipStream_t)stream, z, rows, n, (long)ldz, bn_part, tiles);
    else
        hipLaunchKernelGGL(col_stats_kernel, dim3(xv_cdiv(n, 32), tiles), dim3(256), 0, (hipStream_t)stream, z, rows, n, (long)ldz, bn_part, tiles);
    XV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------
// Activation context (network_relu_type, tdnn.py:24-30 / common.py:27-42): the non-linearity behind a BatchNorm is
//   act(y) = y > 0 ? y : slope[c] * y     slope = NULL: ReLU | a constant 0.2 vector: tf.nn.leaky_relu | the layer's alpha: prelu
// (prelu(x) = relu(x) + alpha (x - |x|) / 2 is exactly that).  The engine sets the context around a layer's calls; every entry
// point with a `relu` flag reads it, so the C signatures stay as they are.  dalpha: where the backward entry points write
// d alpha[c] = sum_rows d act * min(y, 0) (prelu only).
// ------------------------------------------------------------------------------------
static thread_local XvActContext g_act = {nullptr, nullptr};
void xv_set_act_context(const float* slope, float* dalpha) { g_act.slope = slope; g_act.dalpha = dalpha; }
XvActContext xv_act_context() { return g_act; }
extern "C" int xv_set_activation(const float* slope, float* dalpha) {
    XV_REQUIRE(slope || !dalpha, "set_activation: a d alpha buffer needs a slope vector");
    xv_set_act_context(slope, dalpha);
    return 0;
}

// ------------------------------------------------------------------------------------
// BatchNorm
// ------------------------------------------------------------------------------------
// block = 256 threads = 8 channels x 32 tile lanes (n/8 workgroups: the partials are few, the latency of a
// serial walk over them is what this kernel costs).  Each lane folds its tiles' (count, mean, M2) with Chan's
// pairwise formula in double, lanes are then folded in lane order (deterministic).
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ part, int rows, int n, int tiles,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float momentum, int unbiased, float* __restrict__ mmean,
                                                          float* __restrict__ mvar, float* __restrict__ mean_o,
                                                          float* __restrict__ invstd_o, float* __restrict__ scale_o,
                                                          float* __restrict__ shift_o, float* __restrict__ zmin_o,
                                                          float* __restrict__ zmax_o, unsigned* __restrict__ amax_o, int relu,
                                                          const float* __restrict__ slope) {
    XV_EW_PRIORITY();
    __shared__ double s_cnt[FIN_LANES][FIN_CH], s_mean[FIN_LANES][FIN_CH], s_m2[FIN_LANES][FIN_CH];
    __shared__ float s_mn[FIN_LANES][FIN_CH], s_mx[FIN_LANES][FIN_CH];
    const int cx = threadIdx.x & (FIN_CH - 1), tl = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + cx;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    float zmn = INFINITY, zmx = -INFINITY;
    if (c < n) {
        // the loads of FIN_BATCH tiles are issued together, then folded in tile order: the kernel is a chain of memory round trips
        // (7 per lane at S1 when every tile waited for its own four loads: 11.6 us per layer, five layers per step)
        for (int t0 = tl; t0 < tiles; t0 += FIN_LANES * FIN_BATCH) {
            float ps[FIN_BATCH], pq[FIN_BATCH], pmn[FIN_BATCH], pmx[FIN_BATCH];
#pragma unroll
            for (int u = 0; u < FIN_BATCH; ++u) {
                const int t = min(t0 + u * FIN_LANES, tiles - 1);
                ps[u] = part[(long)t * n + c];
                pq[u] = part[((long)tiles + t) * n + c];
                pmn[u] = part[(2L * tiles + t) * n + c];
                pmx[u] = part[(3L * tiles + t) * n + c];
            }
#pragma unroll
            for (int u = 0; u < FIN_BATCH; ++u) {
                const int t = t0 + u * FIN_LANES;
                if (t >= tiles) break;
                zmn = fminf(zmn, pmn[u]);
                zmx = fmaxf(zmx, pmx[u]);
                int tc = min(XV_TILE_M, rows - t * XV_TILE_M);
                double tm = (double)(ps[u] / (float)tc);   // the tile mean the producer centred on
                double tq = (double)pq[u];
                double nn = cnt + (double)tc, d = tm - mean;
                mean += d * ((double)tc / nn);
                m2 += tq + d * d * (cnt * (double)tc / nn);
                cnt = nn;
            }
        }
    }
    s_cnt[tl][cx] = cnt; s_mean[tl][cx] = mean; s_m2[tl][cx] = m2;
    s_mn[tl][cx] = zmn; s_mx[tl][cx] = zmx;
    __syncthreads();
    // fold the 32 lanes of a channel as a tree (lane l takes lane l + stride: a fixed order): the serial fold by lane 0 was 31 dependent
    // Chan merges with two fp64 divisions each - 4 of the kernel's 12 us
    for (int stride = FIN_LANES / 2; stride >= 1; stride >>= 1) {
        if (tl < stride) {
            const double cb = s_cnt[tl + stride][cx];
            if (cb > 0.0) {
                const double nn = cnt + cb, d = s_mean[tl + stride][cx] - mean;
                mean += d * (cb / nn);
                m2 += s_m2[tl + stride][cx] + d * d * (cnt * cb / nn);
                cnt = nn;
            }
            zmn = fminf(zmn, s_mn[tl + stride][cx]);
            zmx = fmaxf(zmx, s_mx[tl + stride][cx]);
            s_cnt[tl][cx] = cnt; s_mean[tl][cx] = mean; s_m2[tl][cx] = m2;
            s_mn[tl][cx] = zmn; s_mx[tl][cx] = zmx;
        }
        __syncthreads();
    }
    if (tl != 0 || c >= n) return;
    float var = (float)(m2 / (double)rows);
    float meanf = (float)mean;
    float invstd = 1.0f / sqrtf(var + eps);
    float sc = gamma[c] * invstd;
    mean_o[c] = meanf;
    invstd_o[c] = invstd;
    const float sh = beta[c] - meanf * sc;
    scale_o[c] = sc;
    shift_o[c] = sh;
    if (zmin_o) { zmin_o[c] = zmn; zmax_o[c] = zmx; }
    if (amax_o) {
        // exact range of y = z*sc + sh over the batch (affine => extremes at the ends), same fma as bn_apply
        float y0 = zmn * sc + sh, y1 = zmx * sc + sh;
        float am = relu ? fmaxf(0.f, fmaxf(y0, y1)) : fmaxf(fabsf(y0), fabsf(y1));
        if (relu && slope) am = fmaxf(fabsf(act1(y0, slope[c])), fabsf(act1(y1, slope[c])));      // piecewise linear through 0: extremes at the ends
        atomicMax(amax_o, __float_as_uint(am));          // max of non-negative floats == max of their bit patterns
    }
    if (mmean) {
        float v = (unbiased && rows > 1) ? var * ((float)rows / (float)(rows - 1)) : var;
        mmean[c] = mmean[c] * momentum + meanf * (1.0f - momentum);
        mvar[c] = mvar[c] * momentum + v * (1.0f - momentum);
    }
}

extern "C" int xv_bn_finalize(void* stream, const float* bn_part, int rows, int n, const float* gamma, const float* beta,
                              float eps, float momentum, int unbiased_moving, float* moving_mean, float* moving_var,
                              float* mean, float* invstd, float* scale, float* shift, float* zmin, float* zmax,
                              uint32_t* amax, int relu) {
    XV_REQUIRE(rows > 0 && n > 0, "bn_finalize: bad shape");
    int tiles = xv_cdiv(rows, XV_TILE_M);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(xv_cdiv(n, FIN_CH)), dim3(256), 0, (hipStream_t)stream, bn_part, rows, n, tiles,
                       gamma, beta, eps, momentum, unbiased_moving, moving_mean, moving_var, mean, invstd, scale, shift, zmin, zmax, amax, relu,
                       g_act.slope);
    XV_LAUNCH_CHECK();
    return 0;
}

// Range of z per channel from the GEMM epilogue's min/max partials and the exact output range of
// relu?(z*scale+shift) for given (e.g. inference) scale/shift: *amax |= its float bits.
__global__ void bn_output_range_kernel(const float* __restrict__ part, int rows, int n, int tiles, const float* __restrict__ scale,
                                       const float* __restrict__ shift, int relu, float* __restrict__ zmin_o,
                                       float* __restrict__ zmax_o, unsigned* __restrict__ amax_o, const float* __restrict__ slope) {
    XV_EW_PRIORITY();
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int t = 0; t < tiles; ++t) {
        mn = fminf(mn, part[(2L * tiles + t) * n + c]);
        mx = fmaxf(mx, part[(3L * tiles + t) * n + c]);
    }
    if (zmin_o) { zmin_o[c] = mn; zmax_o[c] = mx; }
    float y0 = mn * scale[c] + shift[c], y1 = mx * scale[c] + shift[c];
    float am = relu ? fmaxf(0.f, fmaxf(y0, y1)) : fmaxf(fabsf(y0), fabsf(y1));
    if (relu && slope) am = fmaxf(fabsf(act1(y0, slope[c])), fabsf(act1(y1, slope[c])));
    atomicMax(amax_o, __float_as_uint(am));
}

extern "C" int xv_bn_output_range(void* stream, const float* bn_part, int rows, int n, const float* scale, const float* shift, int relu,
                                  float* zmin, float* zmax, uint32_t* amax) {
    XV_REQUIRE(bn_part && rows > 0 && n > 0 && scale && shift && amax, "bn_output_range: bad arguments");
    int tiles = xv_cdiv(rows, XV_TILE_M);
    hipLaunchKernelGGL(bn_output_range_kernel, dim3(xv_cdiv(n, 128)), dim3(128), 0, (hipStream_t)stream, bn_part, rows, n, tiles, scale, shift,
                       relu, zmin, zmax, (unsigned*)amax, g_act.slope);
    XV_LAUNCH_CHECK();
    return 0;
}

__global__ void bn_inference_scale_kernel(int n, const float* __restrict__ gamma, const float* __restrict__ beta,
                                          const float* __restrict__ mmean, const float* __restrict__ mvar, float eps,
                                          float* __restrict__ scale, float* __restrict__ shift) {
    XV_EW_PRIORITY();
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    float sc = gamma[c] * (1.0f / sqrtf(mvar[c] + eps));
    scale[c] = sc;
    shift[c] = beta[c] - mmean[c] * sc;
}

extern "C" int xv_bn_inference_scale(void* stream, int n, const float* gamma, const float* beta, const float* moving_mean,
                                     const float* moving_var, float eps, float* scale, float* shift) {
    XV_REQUIRE(n > 0, "bn_inference_scale: bad shape");
    hipLaunchKernelGGL(bn_inference_scale_kernel, dim3(xv_cdiv(n, 128)), dim3(128), 0, (hipStream_t)stream, n, gamma, beta,
                       moving_mean, moving_var, eps, scale, shift);
    XV_LAUNCH_CHECK();
    return 0;
}

// a = relu?(z*scale+shift).  Thread = one channel quad (16 B) x a strip of rows, block = 64 quads x 4 row lanes over BA_ROWS rows: scale,
// shift and slope are loaded once per thread and the strip's eight loads are in flight together (the element-per-thread grid-stride form
// divided by the row length and reloaded the three vectors for every 16 bytes: 34 us for 97.5 MB alone, r02_elementwise.json).
#define BA_ROWS 32
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, int rows, int nq, long ldz, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, int relu, float* __restrict__ a, long lda,
                                                       const float* __restrict__ slope) {
    XV_EW_PRIORITY();
    const int q = blockIdx.y * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    if (q >= nq) return;
    const f32x4 sc = *(const f32x4*)(scale + 4 * q), sh = *(const f32x4*)(shift + 4 * q);
    f32x4 sl = {0, 0, 0, 0};
    if (slope) sl = *(const f32x4*)(slope + 4 * q);
    const int r0 = blockIdx.x * BA_ROWS + rl;
    f32x4 v[BA_ROWS / 4];
#pragma unroll
    for (int j = 0; j < BA_ROWS / 4; ++j) v[j] = *(const f32x4*)(z + (long)min(r0 + 4 * j, rows - 1) * ldz + 4 * q);
#pragma unroll
    for (int j = 0; j < BA_ROWS / 4; ++j) {
        f32x4 y = v[j] * sc + sh;
        if (relu) y = slope ? act4(y, sl) : relu4(y);
        if (r0 + 4 * j < rows) *(f32x4*)(a + (long)(r0 + 4 * j) * lda + 4 * q) = y;
    }
}

extern "C" int xv_bn_apply(void* stream, const float* z, int rows, int n, int ldz, const float* scale, const float* shift,
                           int relu, float* a, int lda) {
    XV_REQUIRE(rows > 0 && n > 0 && n % 4 == 0 && ldz % 4 == 0 && lda % 4 == 0, "bn_apply: n/ld must be multiples of 4 (n=%d)", n);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(xv_cdiv(rows, BA_ROWS), xv_cdiv(n / 4, 64)), dim3(256), 0, (hipStream_t)stream, z, rows, n / 4,
                       (long)ldz, scale, shift, relu, a, (long)lda, g_act.slope);
    XV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------
// small-row BatchNorm, one launch (xv_bn.h).  block = 256 threads = 16 channels x 16 row lanes; fixed-order combines.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float small_reduce16(float v, float (*red)[16], int rl, int cx) {
    __syncthreads();
    red[rl][cx] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][cx];
    return t;
}

__global__ __launch_bounds__(256) void bn_small_fwd_kernel(const float* __restrict__ z, int rows, int n, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float momentum, int unbiased,
                                                           float* __restrict__ mmean, float* __restrict__ mvar, float* __restrict__ mean_o,
                                                           float* __restrict__ invstd_o, float* __restrict__ scale_o,
                                                           float* __restrict__ shift_o, int relu, float* __restrict__ a,
                                                           const float* __restrict__ slope) {
    XV_EW_PRIORITY();
    __shared__ float red[16][16];
    const int cx = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    const bool cv = c < n;
    float s = 0.f;
    if (cv) for (int r = rl; r < rows; r += 16) s += z[(long)r * n + c];
    const float mean = small_reduce16(s, red, rl, cx) / (float)rows;
    float q = 0.f;
    if (cv) for (int r = rl; r < rows; r += 16) { float d = z[(long)r * n + c] - mean; q += d * d; }
    const float var = small_reduce16(q, red, rl, cx) / (float)rows;      // biased, two-pass (tf.nn.moments)
    if (!cv) return;
    const float invstd = 1.0f / sqrtf(var + eps);
    const float sc = gamma[c] * invstd, sh = beta[c] - mean * sc;
    if (rl == 0) {
        mean_o[c] = mean; invstd_o[c] = invstd; scale_o[c] = sc; shift_o[c] = sh;
        if (mmean) {
            float v = (unbiased && rows > 1) ? var * ((float)rows / (float)(rows - 1)) : var;
            mmean[c] = mmean[c] * momentum + mean * (1.0f - momentum);
            mvar[c] = mvar[c] * momentum + v * (1.0f - momentum);
        }
    }
    if (a)
        for (int r = rl; r < rows; r += 16) {
            float y = z[(long)r * n + c] * sc + sh;
            a[(long)r * n + c] = relu ? (slope ? act1(y, slope[c]) : fmaxf(y, 0.f)) : y;
        }
}

int xv_bn_small_forward(hipStream_t s, const float* z, int rows, int n, const float* gamma, const float* beta, float eps, float momentum,
                        int unbiased_moving, float* moving_mean, float* moving_var, float* mean, float* invstd, float* scale, float* shift,
                        int relu, float* a) {
    XV_REQUIRE(rows > 0 && rows <= XV_BN_SMALL_MAX_ROWS && n > 0, "bn_small_forward: bad shape (rows=%d)", rows);
    hipLaunchKernelGGL(bn_small_fwd_kernel, dim3(xv_cdiv(n, 16)), dim3(256), 0, s, z, rows, n, gamma, beta, eps, momentum, unbiased_moving,
                       moving_mean, moving_var, mean, invstd, scale, shift, relu, a, relu ? xv_act_context().slope : nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void bn_small_bwd_kernel(const float* __restrict__ da, const float* __restrict__ z, int rows, int n,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, int relu, float* __restrict__ dz,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ dbias, const float* __restrict__ slope,
                                                           float* __restrict__ dalpha) {
    XV_EW_PRIORITY();
    __shared__ float red[16][16];
    const int cx = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    const bool cv = c < n;
    float mu = 0.f, is = 0.f, sc = 0.f, sh = 0.f, sl = 0.f;
    if (cv) { mu = mean[c]; is = invstd[c]; sc = scale[c]; sh = shift[c]; sl = slope ? slope[c] : 0.f; }
    float s1 = 0.f, s2 = 0.f, s4 = 0.f;
    if (cv)
        for (int r = rl; r < rows; r += 16) {
            float zz = z[(long)r * n + c], dd = da[(long)r * n + c];
            const float y = zz * sc + sh;
            if (relu) { s4 += dd * fminf(y, 0.f); if (!(y > 0.f)) dd *= sl; }
            s1 += dd;
            s2 += dd * ((zz - mu) * is);
        }
    s1 = small_reduce16(s1, red, rl, cx);
    s2 = small_reduce16(s2, red, rl, cx);
    if (dalpha) s4 = small_reduce16(s4, red, rl, cx);      // (uniform: every thread of the block takes the same path)
    if (!cv) return;
    const float c1 = s1 / (float)rows, c2 = s2 / (float)rows;
    const float g = gamma[c] * is;
    if (rl == 0) {
        dbeta[c] = s1; dgamma[c] = s2;
        if (dbias) dbias[c] = g * (s1 - c1 * (float)rows);
        if (dalpha) dalpha[c] = s4;
    }
    for (int r = rl; r < rows; r += 16) {
        float zz = z[(long)r * n + c], dd = da[(long)r * n + c];
        if (relu && !(zz * sc + sh > 0.f)) dd *= sl;
        dz[(long)r * n + c] = g * (dd - c1 - ((zz - mu) * is) * c2);
    }
}

int xv_bn_small_backward(hipStream_t s, const float* da, const float* z, int rows, int n, const float* gamma, const float* mean,
                         const float* invstd, const float* scale, const float* shift, int relu, float* dz, float* dgamma, float* dbeta,
                         float* dbias) {
    XV_REQUIRE(rows > 0 && rows <= XV_BN_SMALL_MAX_ROWS && n > 0, "bn_small_backward: bad shape (rows=%d)", rows);
    const XvActContext act = xv_act_context();
    hipLaunchKernelGGL(bn_small_bwd_kernel, dim3(xv_cdiv(n, 16)), dim3(256), 0, s, da, z, rows, n, gamma, mean, invstd, scale, shift, relu,
                       dz, dgamma, dbeta, dbias, relu ? act.slope : nullptr, (relu && act.slope) ? act.dalpha : nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}

__global__ void relu_bwd_kernel(const float* __restrict__ da, const float* __restrict__ a, size_t count, float* __restrict__ dz) {
    XV_EW_PRIORITY();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        dz[i] = a[i] > 0.f ? da[i] : 0.f;
}
// The same with a slope (act context): forward a = act(z) and backward dz = da * act'(z), d alpha[c] = sum_r da * min(z, 0); rows <= XV_BN_SMALL_MAX_ROWS
__global__ __launch_bounds__(256) void act_small_kernel(const float* __restrict__ da, const float* __restrict__ z, int rows, int n,
                                                        const float* __restrict__ slope, float* __restrict__ out,
                                                        float* __restrict__ dalpha) {
    XV_EW_PRIORITY();
    __shared__ float red[16][16];
    const int cx = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cx;
    const bool cv = c < n;
    const float sl = cv ? slope[c] : 0.f;
    float s4 = 0.f;
    if (cv)
        for (int r = rl; r < rows; r += 16) {
            const float zz = z[(long)r * n + c];
            if (da) {
                const float dd = da[(long)r * n + c];
                s4 += dd * fminf(zz, 0.f);
                out[(long)r * n + c] = zz > 0.f ? dd : dd * sl;
            } else {
                out[(long)r * n + c] = act1(zz, sl);
            }
        }
    if (dalpha) {
        s4 = small_reduce16(s4, red, rl, cx);
        if (cv && rl == 0) dalpha[c] = s4;
    }
}
int xv_act_small(hipStream_t s, const float* da, const float* z, int rows, int n, float* out) {
    const XvActContext act = xv_act_context();
    XV_REQUIRE(act.slope && rows > 0 && rows <= XV_BN_SMALL_MAX_ROWS && n > 0, "act_small: needs an activation slope and a segment-level tensor");
    hipLaunchKernelGGL(act_small_kernel, dim3(xv_cdiv(n, 16)), dim3(256), 0, s, da, z, rows, n, act.slope, out, da ? act.dalpha : (float*)nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}

// y[r][c] = x > 0 ? x : alpha[c] * x  (common.py:27-42 prelu = relu(x) + alpha (x - |x|) / 2; a constant alpha = leaky ReLU)
__global__ void prelu_fwd_kernel(const float* __restrict__ x, size_t count, int n, const float* __restrict__ alpha, float* __restrict__ y) {
    XV_EW_PRIORITY();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) y[i] = act1(x[i], alpha[i % n]);
}
extern "C" int xv_prelu_forward(void* stream, const float* x, int rows, int n, const float* alpha, float* y) {
    XV_REQUIRE(x && alpha && y && rows > 0 && n > 0, "prelu_forward: bad arguments");
    const size_t count = (size_t)rows * n;
    hipLaunchKernelGGL(prelu_fwd_kernel, dim3(grid_for((long)count, 256)), dim3(256), 0, (hipStream_t)stream, x, count, n, alpha, y);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_relu_backward(void* stream, const float* da, const float* a, size_t count, float* dz) {
    XV_REQUIRE(count > 0, "relu_backward: empty");
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for((long)count, 256)), dim3(256), 0, (hipStream_t)stream, da, a, count, dz);
    XV_LAUNCH_CHECK();
    return 0;
}
