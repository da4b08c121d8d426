// Helpers shared by the element-wise units (xv_runtime, xv_prep, xv_bn, xv_bn_bwd, xv_pool, xv_update) and by the activation
// sites of xv_planes16.hip and xv_attention.hip: the launch grid of a grid-stride kernel, the wave sum, and the activation behind a
// BatchNorm (act context, below) on a channel quad, forward and backward.  Device helpers are all __forceinline__: every kernel
// keeps the instruction sequence it had with the expression written out.
#pragma once
#include "xv_common.h"

// Activation behind a BatchNorm in the layer being processed (network_relu_type, tdnn.py:24-30): y > 0 ? y : slope[c] * y.
// slope == nullptr: ReLU.  Set by the engine around a layer's calls (prelu: the layer's alpha variable, with dalpha = its gradient;
// lrelu: a constant 0.2 vector); every entry point that takes a `relu` flag reads it (xv_bn.hip owns it).
struct XvActContext { const float* slope; float* dalpha; };
void xv_set_act_context(const float* slope, float* dalpha);
XvActContext xv_act_context();

// *out += scale * sum(w[0 .. count)^2) by a fixed-order two-stage reduction (xv_update.hip); part: XV_SUMSQ_PARTS floats of scratch
#define XV_SUMSQ_PARTS 512
int xv_sumsq_ordered(hipStream_t s, const float* w, size_t count, float scale, float* out, float* part);
// g[0 .. count) *= grad_scale * clip / max(grad_scale * sqrt(*sumsq), clip)   (tf.clip_by_global_norm; xv_update.hip)
int xv_clip_scale(hipStream_t s, float* g, size_t count, const float* sumsq, float grad_scale, float clip);

// Geometry of the two kernels that finalise per-channel statistics from partials (bn_finalize_kernel, bn_bwd_finalize_kernel): a block of
// 256 threads = FIN_CH channels x FIN_LANES partial lanes, FIN_BATCH partials' loads in flight per lane
#define FIN_CH 8
#define FIN_LANES 32
#define FIN_BATCH 8

static inline int grid_for(long total, int block, int cap = 4096) {
    long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// butterfly: a + b and b + a are the same bits, so every lane holds one value
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// act(y) = y > 0 ? y : slope * y
__device__ __forceinline__ float act1(float y, float sl) { return y > 0.f ? y : y * sl; }
__device__ __forceinline__ f32x4 act4(f32x4 y, f32x4 sl) {
    f32x4 r;
    r.x = act1(y.x, sl.x); r.y = act1(y.y, sl.y); r.z = act1(y.z, sl.z); r.w = act1(y.w, sl.w);
    return r;
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    return v;
}
__device__ __forceinline__ f32x4 neg4(f32x4 y) {      // min(y, 0)
    f32x4 r;
    r.x = fminf(y.x, 0.f); r.y = fminf(y.y, 0.f); r.z = fminf(y.z, 0.f); r.w = fminf(y.w, 0.f);
    return r;
}
// the gradient dd behind the activation of y: dd where the unit is on, dd * slope (hs: the activation has a slope) or 0 where it is off
__device__ __forceinline__ f32x4 mask_grad4(f32x4 dd, f32x4 y, f32x4 sl, bool hs) {
    if (hs) {
        dd.x = y.x > 0.f ? dd.x : dd.x * sl.x; dd.y = y.y > 0.f ? dd.y : dd.y * sl.y;
        dd.z = y.z > 0.f ? dd.z : dd.z * sl.z; dd.w = y.w > 0.f ? dd.w : dd.w * sl.w;
    } else {
        dd.x = y.x > 0.f ? dd.x : 0.f; dd.y = y.y > 0.f ? dd.y : 0.f;
        dd.z = y.z > 0.f ? dd.z : 0.f; dd.w = y.w > 0.f ? dd.w : 0.f;
    }
    return dd;
}
__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
    a.x = fmaxf(a.x, b.x); a.y = fmaxf(a.y, b.y); a.z = fmaxf(a.z, b.z); a.w = fmaxf(a.w, b.w);
    return a;
}
// running max |v| per component
__device__ __forceinline__ f32x4 absmax4(f32x4 acc, f32x4 v) {
    acc.x = fmaxf(acc.x, fabsf(v.x)); acc.y = fmaxf(acc.y, fabsf(v.y));
    acc.z = fmaxf(acc.z, fabsf(v.z)); acc.w = fmaxf(acc.w, fabsf(v.w));
    return acc;
}
