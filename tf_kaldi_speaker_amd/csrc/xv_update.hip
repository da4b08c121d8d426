// What turns a step's gradients into new variables: column sums (bias gradients), the fixed-order sum of squares (l2 loss,
// clip-by-global-norm) and the optimisers.  fp32, reductions are row-chunk / block partials followed by a fixed-order combine: no
// atomics on any path that feeds a gradient.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"

// ------------------------------------------------------------------------------------
// column sums / column statistics (row-chunk partials, then a fixed-order combine)
// ------------------------------------------------------------------------------------
#define CS_ROWS 128
// block = 256 threads = 64 columns x 4 row lanes; row lanes are combined in a fixed order
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ a, int rows, int n, long lda,
                                                             float* __restrict__ part) {
    XV_EW_PRIORITY();
    __shared__ float red[4][64];
    const int cx = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cx;
    const int r0 = blockIdx.y * CS_ROWS, r1 = min(rows, r0 + CS_ROWS);
    float s = 0.f;
    if (col < n) {
        int r = r0 + rl;
        for (; r + 12 < r1; r += 16) {
            float v0 = a[(long)r * lda + col], v1 = a[(long)(r + 4) * lda + col];
            float v2 = a[(long)(r + 8) * lda + col], v3 = a[(long)(r + 12) * lda + col];
            s += (v0 + v1) + (v2 + v3);
        }
        for (; r < r1; r += 4) s += a[(long)r * lda + col];
    }
    red[rl][cx] = s;
    __syncthreads();
    if (rl == 0 && col < n) part[(long)blockIdx.y * n + col] = (red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx]);
}
// block = 256 threads = 32 columns x 8 chunk lanes
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ part, int chunks, int n, float* __restrict__ out) {
    XV_EW_PRIORITY();
    __shared__ float red[8][32];
    const int cx = threadIdx.x & 31, cl = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cx;
    float s = 0.f;
    if (col < n)
        for (int c = cl; c < chunks; c += 8) s += part[(long)c * n + col];
    red[cl][cx] = s;
    __syncthreads();
    if (cl == 0 && col < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][cx];
        out[col] = t;
    }
}

extern "C" int xv_colsum(void* stream, const float* a, int rows, int n, int lda, float* out, void* ws, size_t ws_bytes) {
    XV_REQUIRE(rows > 0 && n > 0 && lda >= n, "colsum: bad shape");
    int chunks = xv_cdiv(rows, CS_ROWS);
    XV_REQUIRE((size_t)chunks * n * sizeof(float) <= ws_bytes, "colsum: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(xv_cdiv(n, 64), chunks), dim3(256), 0, s, a, rows, n, (long)lda, (float*)ws);
    XV_LAUNCH_CHECK();
    hipLaunchKernelGGL(colsum_final_kernel, dim3(xv_cdiv(n, 32)), dim3(256), 0, s, (const float*)ws, chunks, n, out);
    XV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------
// scalar reductions (reporting / clip-by-global-norm only) and optimisers
// ------------------------------------------------------------------------------------
// Fixed-order sum of squares: every block leaves its partial in part[blockIdx.x], then one block adds the partials in index order
// (as colsum_partial_kernel / colsum_final_kernel do).  The result is the same bits on every run and on every rank: with
// clip_gradient_norm > 0 the clip scale is a function of it, and replicas, a resumed run and a replayed step must not drift apart
// over the arrival order of float atomics.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ w, size_t count, float* __restrict__ part) {
    XV_EW_PRIORITY();
    __shared__ float red[4];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) s += w[i] * w[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* __restrict__ part, int nparts, float scale, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out += scale * ((red[0] + red[1]) + (red[2] + red[3]));
}
// *out += scale * sum(w^2); part: XV_SUMSQ_PARTS floats of scratch owned by the caller's stream
int xv_sumsq_ordered(hipStream_t s, const float* w, size_t count, float scale, float* out, float* part) {
    XV_REQUIRE(count > 0 && w && out && part, "sumsq: bad arguments");
    const int nb = grid_for((long)count, 256, XV_SUMSQ_PARTS);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, w, count, part);
    XV_LAUNCH_CHECK();
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, (const float*)part, nb, scale, out);
    XV_LAUNCH_CHECK();
    return 0;
}
// the C-ABI forms own no workspace: a stream-ordered allocation carries the partials
static int sumsq_with_scratch(hipStream_t s, const float* w, size_t count, float scale, float* out) {
    float* part = nullptr;
    XV_CHECK_HIP(hipMallocAsync((void**)&part, XV_SUMSQ_PARTS * sizeof(float), s));
    const int rc = xv_sumsq_ordered(s, w, count, scale, out, part);
    XV_CHECK_HIP(hipFreeAsync(part, s));
    return rc;
}
extern "C" int xv_l2_reg_loss(void* stream, const float* w, size_t count, float scale, float* out_accum) {
    XV_REQUIRE(count > 0, "l2_reg_loss: empty");
    return sumsq_with_scratch((hipStream_t)stream, w, count, 0.5f * scale, out_accum);
}
extern "C" int xv_sumsq(void* stream, const float* g, size_t count, float* out_accum) {
    XV_REQUIRE(count > 0, "sumsq: empty");
    return sumsq_with_scratch((hipStream_t)stream, g, count, 1.0f, out_accum);
}

__global__ void clip_scale_kernel(float* __restrict__ g, size_t count, const float* __restrict__ sumsq, float grad_scale, float clip) {
    // tf.clip_by_global_norm: g * clip / max(norm, clip)
    float norm = sqrtf(*sumsq) * grad_scale;
    float k = grad_scale * (clip / fmaxf(norm, clip));
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) g[i] *= k;
}
// g *= grad_scale * clip / max(grad_scale * sqrt(*sumsq), clip): the engine's clip-by-global-norm, *sumsq from xv_sumsq_ordered
int xv_clip_scale(hipStream_t s, float* g, size_t count, const float* sumsq, float grad_scale, float clip) {
    hipLaunchKernelGGL(clip_scale_kernel, dim3(2048), dim3(256), 0, s, g, count, sumsq, grad_scale, clip);
    XV_LAUNCH_CHECK();
    return 0;
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, size_t count, float lr, float gs) {
    XV_EW_PRIORITY();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        p[i] = p[i] - lr * (g[i] * gs);
}
__global__ void momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ acc, size_t count, float lr,
                                float mom, int nesterov, float gs) {
    XV_EW_PRIORITY();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        float gi = g[i] * gs;
        float a = mom * acc[i] + gi;
        acc[i] = a;
        p[i] = nesterov ? p[i] - lr * (gi + mom * a) : p[i] - lr * a;
    }
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            size_t count, float lr_t, float b1, float b2, float eps, float gs) {
    XV_EW_PRIORITY();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        float gi = g[i] * gs;
        float mi = b1 * m[i] + (1.f - b1) * gi;
        float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
    }
}
extern "C" int xv_sgd_update(void* stream, float* p, const float* g, size_t count, float lr, float grad_scale) {
    XV_REQUIRE(count > 0, "sgd_update: empty");
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for((long)count, 256, 8192)), dim3(256), 0, (hipStream_t)stream, p, g, count, lr, grad_scale);
    XV_LAUNCH_CHECK();
    return 0;
}
extern "C" int xv_momentum_update(void* stream, float* p, const float* g, float* acc, size_t count, float lr, float momentum,
                                  int nesterov, float grad_scale) {
    XV_REQUIRE(count > 0, "momentum_update: empty");
    hipLaunchKernelGGL(momentum_kernel, dim3(grid_for((long)count, 256, 8192)), dim3(256), 0, (hipStream_t)stream, p, g, acc, count, lr,
                       momentum, nesterov, grad_scale);
    XV_LAUNCH_CHECK();
    return 0;
}
extern "C" int xv_adam_update(void* stream, float* p, const float* g, float* m, float* v, size_t count, float lr, float beta1,
                              float beta2, float eps, int t, float grad_scale) {
    XV_REQUIRE(count > 0 && t >= 1, "adam_update: bad arguments");
    double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for((long)count, 256, 8192)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, count,
                       (float)lr_t, beta1, beta2, eps, grad_scale);
    XV_LAUNCH_CHECK();
    return 0;
}
