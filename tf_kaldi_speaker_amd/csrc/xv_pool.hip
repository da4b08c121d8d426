// Statistics pooling (plain, or fused with the last frame layer's BatchNorm + activation; optional attention weights) and
// l2_scaling.  A wave reads whole channel quads of one frame; reductions over frames are Welford / Chan merges in a fixed order.
// (The BatchNorm backward that evaluates the pooling backward on the fly is in xv_bn_bwd.hip.)  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_bn.h"      // XvBnUpstream
#include "xv_pool.h"

// ------------------------------------------------------------------------------------
// statistics pooling (pooling.py:9-34)
// wave = 64 channel-quads of one frame, block = 4 waves = 4 frame lanes.  Each lane runs Welford over its frames for 4 channels (two
// interleaved chains); chains and waves are merged with Chan's formula (through LDS across waves).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void wf_merge(f32x4& mean, f32x4& m2, float& n, const f32x4& mean_b, const f32x4& m2_b, float n_b) {
    float nn = n + n_b;
    if (nn > 0.f) {
        f32x4 d = mean_b - mean;
        float w = n_b / nn;
        mean = mean + d * w;
        m2 = m2 + m2_b + d * d * (n * w);
    }
    n = nn;
}

// BN: the pooled tensor is relu?(x*scale + shift) evaluated on the fly (x = the pre-BN output of the last frame layer), so the
// activation is never written to memory.
// A wave reads ONE contiguous KiB per instruction (64 channel quads of one frame), the 4 waves are 4 frame lanes, every lane keeps 8
// loads in flight and runs TWO Welford chains (alternate frames of its lane), merged at the end.  [measured, S1: 143 MB] 33 us warm
// (Infinity Cache) / 54 us cold with event overhead - what a plain streaming read of the tensor takes (own amax kernel 32 / 53 us,
// torch.sum 35 / 60 us); the first form (32 quads x 8 frame lanes, 4 loads, one chain) took 41 / 61 us.
template <bool BN>
__global__ __launch_bounds__(256) void stat_pool_fwd_kernel(const float* __restrict__ x, int T, int C, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int relu, const float* __restrict__ wts,
                                                            float* __restrict__ out, const float* __restrict__ slope,
                                                            float* __restrict__ wpos, float* __restrict__ amax_o,
                                                            const int* __restrict__ flen, int shrink, int ld /* floats per row of x (>= C) */) {
    XV_EW_PRIORITY();
    __shared__ f32x4 s_mean[4][64], s_m2[4][64], s_wp[4][64], s_mx[4][64];
    __shared__ float s_n[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * 4;
    const int b = blockIdx.y;
    const bool cv = col < C;
    const float* xp = x + (long)b * T * ld + (cv ? col : 0);
    // flen (batched extraction): chunk b holds flen[b] - shrink valid frames, the rest of its T rows is padding that is not pooled
    const int Tstride = T;
    if (flen) T = max(1, min(T, flen[b] - shrink));
    f32x4 sc = {1, 1, 1, 1}, sh = {0, 0, 0, 0}, sl = {0, 0, 0, 0};
    const bool hs = BN && slope != nullptr;
    if (BN && cv) { sc = *(const f32x4*)(scale + col); sh = *(const f32x4*)(shift + col); if (hs) sl = *(const f32x4*)(slope + col); }
    auto act = [&](f32x4 v) {
        if (BN) {
            v = v * sc + sh;
            if (relu) v = hs ? act4(v, sl) : relu4(v);
        }
        return v;
    };
    const float* wp = wts ? wts + (long)b * Tstride : nullptr;
    f32x4 mean0 = {0, 0, 0, 0}, m20 = {0, 0, 0, 0}, mean1 = {0, 0, 0, 0}, m21 = {0, 0, 0, 0};
    f32x4 wpp = {0, 0, 0, 0};       // sum of the frame weights where the activation is on (all frames without a ReLU)
    const bool cnt_all = !(BN && relu);
    f32x4 amx = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    auto on = [&](f32x4 a, float w) {
        wpp.x += (cnt_all || a.x > 0.f) ? w : 0.f; wpp.y += (cnt_all || a.y > 0.f) ? w : 0.f;
        wpp.z += (cnt_all || a.z > 0.f) ? w : 0.f; wpp.w += (cnt_all || a.w > 0.f) ? w : 0.f;
        if (amax_o) { amx.x = fmaxf(amx.x, a.x); amx.y = fmaxf(amx.y, a.y); amx.z = fmaxf(amx.z, a.z); amx.w = fmaxf(amx.w, a.w); }      // (split precision only)
    };
    float n0 = 0.f, n1 = 0.f;
    // frame weights: 1 (statistics pooling; n counts frames) or the attention weights of this chunk (n sums them); weighted incremental
    // mean / M2 (West), identical to Welford for unit weights.  Unit weights: 1 / n through v_rcp_f32 (1 ulp, exact for n = 1) - the
    // IEEE division sequence sat on the serial mean -> M2 chain of every frame and made this pass VALU-latency-bound.  Attention weights
    // keep the exact quotient: there w / n must be exactly 1 on a lane's first frame, or a constant chunk no longer has a zero variance
    // (reference test_utils.py / pooling.py:160-162 clamp).
#define XV_POOL_STEP2(mean, m2, n, v, w) { n += (w); const f32x4 d_ = (v) - mean; if (n > 0.f) mean += d_ * (wp ? (w) / n : __builtin_amdgcn_rcpf(n)); m2 += d_ * ((v) - mean) * (w); }
    // [measured, round 6] two batches of four loads in flight (the next batch issued before the current one is folded): 26.4 us alone against
    // 26.5 for this form; two batches of eight need 204 VGPRs (a workgroup less per CU)
    int t = wave;
    for (; t + 28 < T; t += 32) {
        f32x4 v[8];
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *(const f32x4*)(xp + (long)(t + 4 * u) * ld);
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = wp ? wp[t + 4 * u] : 1.f;
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            const f32x4 a0 = act(v[u]), a1 = act(v[u + 1]);
            XV_POOL_STEP2(mean0, m20, n0, a0, w[u])
            XV_POOL_STEP2(mean1, m21, n1, a1, w[u + 1])
            if (wpos) { on(a0, w[u]); on(a1, w[u + 1]); }
        }
    }
    for (; t < T; t += 4) {
        const f32x4 a0 = act(*(const f32x4*)(xp + (long)t * ld));
        const float w0 = wp ? wp[t] : 1.f;
        XV_POOL_STEP2(mean0, m20, n0, a0, w0)
        if (wpos) on(a0, w0);
    }
#undef XV_POOL_STEP2
    wf_merge(mean0, m20, n0, mean1, m21, n1);
    s_mean[wave][lane] = mean0;
    s_m2[wave][lane] = m20;
    s_wp[wave][lane] = wpp;
    s_mx[wave][lane] = amx;
    if (lane == 0) s_n[wave] = n0;
    __syncthreads();
    if (wave == 0 && cv) {
        f32x4 mean = s_mean[0][lane], m2 = s_m2[0][lane];
        float n = s_n[0];
        for (int w = 1; w < 4; ++w) wf_merge(mean, m2, n, s_mean[w][lane], s_m2[w][lane], s_n[w]);
        if (wpos) *(f32x4*)(wpos + (long)b * C + col) = ((s_wp[0][lane] + s_wp[1][lane]) + (s_wp[2][lane] + s_wp[3][lane])) * (1.f / n);
        if (amax_o) {
            f32x4 mx = s_mx[0][lane];
            for (int w = 1; w < 4; ++w) {
                mx = max4(mx, s_mx[w][lane]);
            }
            *(f32x4*)(amax_o + (long)b * C + col) = mx;
        }
        f32x4 var = m2 * (1.f / n);
        const float eps = 1e-12f;
        f32x4 sd;
        sd.x = sqrtf(var.x <= eps ? eps : var.x); sd.y = sqrtf(var.y <= eps ? eps : var.y);
        sd.z = sqrtf(var.z <= eps ? eps : var.z); sd.w = sqrtf(var.w <= eps ? eps : var.w);
        *(f32x4*)(out + (long)b * 2 * C + col) = mean;
        *(f32x4*)(out + (long)b * 2 * C + C + col) = sd;
    }
}

extern "C" int xv_stat_pool_forward(void* stream, const float* x, int b, int t, int c, float* out) {
    XV_REQUIRE(b > 0 && t > 0 && c > 0 && c % 4 == 0, "stat_pool_forward: bad shape (c=%d must be a multiple of 4)", c);
    hipLaunchKernelGGL(stat_pool_fwd_kernel<false>, dim3(xv_cdiv(c / 4, 64), b), dim3(256), 0, (hipStream_t)stream, x, t, c,
                       (const float*)nullptr, (const float*)nullptr, 0, (const float*)nullptr, out, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                       (const int*)nullptr, 0, c);
    XV_LAUNCH_CHECK();
    return 0;
}

// wpos, amax (optional, [b][c]): see XvBnUpstream (xv_bn.h)
int xv_stat_pool_forward_bn_ex(hipStream_t s, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                               const float* weights, float* out, float* wpos, float* amax, const int32_t* frames, int shrink, int ldz) {
    XV_REQUIRE(b > 0 && t > 0 && c > 0 && c % 4 == 0 && scale && shift, "stat_pool_forward_bn: bad shape (c=%d must be a multiple of 4)", c);
    if (ldz == 0) ldz = c;
    XV_REQUIRE(ldz >= c && ldz % 4 == 0, "stat_pool_forward_bn: bad row pitch %d", ldz);
    hipLaunchKernelGGL(stat_pool_fwd_kernel<true>, dim3(xv_cdiv(c / 4, 64), b), dim3(256), 0, s, z, t, c, scale, shift,
                       relu, weights, out, relu ? xv_act_context().slope : nullptr, wpos, wpos ? amax : nullptr, (const int*)frames, shrink, ldz);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_stat_pool_forward_bn_aux(void* stream, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                                           const float* weights, float* out, float* wpos, float* amax) {
    XV_REQUIRE(wpos, "stat_pool_forward_bn_aux: wpos is required");
    return xv_stat_pool_forward_bn_ex((hipStream_t)stream, z, b, t, c, scale, shift, relu, weights, out, wpos, amax);
}

extern "C" int xv_stat_pool_forward_bn(void* stream, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                                       const float* weights, float* out) {
    return xv_stat_pool_forward_bn_ex((hipStream_t)stream, z, b, t, c, scale, shift, relu, weights, out, nullptr, nullptr);
}

__global__ void stat_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ out, const float* __restrict__ dout,
                                     int T, int cq, float* __restrict__ dx, long total) {
    XV_EW_PRIORITY();
    const int C = cq * 4;
    const float invT = 1.f / (float)T;
    const float sd_eps = sqrtf(1e-12f);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        long row = i / cq;
        int col = (int)(i - row * cq) * 4;
        int b = (int)(row / T);
        const float* o = out + (long)b * 2 * C;
        const float* g = dout + (long)b * 2 * C;
        f32x4 mean = *(const f32x4*)(o + col), sd = *(const f32x4*)(o + C + col);
        f32x4 dm = *(const f32x4*)(g + col), ds = *(const f32x4*)(g + C + col);
        f32x4 v = *(const f32x4*)(x + row * C + col);
        f32x4 k;   // dstd * (1/std) / T, zero where the variance was clamped (pooling.py:28-29)
        k.x = sd.x <= sd_eps ? 0.f : ds.x / sd.x * invT; k.y = sd.y <= sd_eps ? 0.f : ds.y / sd.y * invT;
        k.z = sd.z <= sd_eps ? 0.f : ds.z / sd.z * invT; k.w = sd.w <= sd_eps ? 0.f : ds.w / sd.w * invT;
        *(f32x4*)(dx + row * C + col) = dm * invT + k * (v - mean);
    }
}

extern "C" int xv_stat_pool_backward(void* stream, const float* x, const float* out, const float* dout, int b, int t, int c, float* dx) {
    XV_REQUIRE(b > 0 && t > 0 && c > 0 && c % 4 == 0, "stat_pool_backward: bad shape");
    long total = (long)b * t * (c / 4);
    hipLaunchKernelGGL(stat_pool_bwd_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, out, dout, t,
                       c / 4, dx, total);
    XV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------
// l2_scaling (common.py:45-58): one wave per row
// ------------------------------------------------------------------------------------
__global__ void l2_scaling_fwd_kernel(const float* __restrict__ x, int rows, int n, float factor, float* __restrict__ y) {
    XV_EW_PRIORITY();
    int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (long)row * n;
    float ss = 0.f;
    for (int c = lane; c < n; c += 64) ss += xr[c] * xr[c];
    ss = wave_sum(ss);
    float inv = rsqrtf(fmaxf(ss, 1e-12f)) * factor;
    for (int c = lane; c < n; c += 64) y[(long)row * n + c] = xr[c] * inv;
}
__global__ void l2_scaling_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, int rows, int n, float factor,
                                      float* __restrict__ dx) {
    XV_EW_PRIORITY();
    int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (long)row * n;
    const float* gr = dy + (long)row * n;
    float ss = 0.f, dot = 0.f;
    for (int c = lane; c < n; c += 64) { ss += xr[c] * xr[c]; dot += xr[c] * gr[c]; }
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    float inv = rsqrtf(fmaxf(ss, 1e-12f)) * factor;
    float k = ss >= 1e-12f ? inv / ss * dot : 0.f;
    for (int c = lane; c < n; c += 64) dx[(long)row * n + c] = gr[c] * inv - xr[c] * k;
}
extern "C" int xv_l2_scaling_forward(void* stream, const float* x, int rows, int n, float factor, float* y) {
    XV_REQUIRE(rows > 0 && n > 0, "l2_scaling_forward: bad shape");
    hipLaunchKernelGGL(l2_scaling_fwd_kernel, dim3(xv_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, n, factor, y);
    XV_LAUNCH_CHECK();
    return 0;
}
extern "C" int xv_l2_scaling_backward(void* stream, const float* x, const float* dy, int rows, int n, float factor, float* dx) {
    XV_REQUIRE(rows > 0 && n > 0, "l2_scaling_backward: bad shape");
    hipLaunchKernelGGL(l2_scaling_bwd_kernel, dim3(xv_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, dy, rows, n, factor, dx);
    XV_LAUNCH_CHECK();
    return 0;
}
