// Producers of the fp16 planes of the split-precision (f16x3) GEMMs: the max |x| reduction behind a tensor's scale, and the two emitters
// (fp32 tensor -> planes; BN + activation of a pre-BN tensor -> planes).  Representation, scale rule and plane layout: xv_gemm16.h.
#include "xv_ew.h"             // grid_for, the act context
#include "xv_gemm16.h"

__device__ __forceinline__ void split_f16(float x, float s, u16& h, u16& l) {
    float xs = x * s;
    _Float16 hh = (_Float16)xs;
    _Float16 ll = (_Float16)(xs - (float)hh);
    h = __builtin_bit_cast(u16, hh);
    l = __builtin_bit_cast(u16, ll);
}

// One atomicMax per WORKGROUP, and only when it can raise the value (same-address atomics serialise in L2:
// thousands of them cost more than the read of the tensor).
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, size_t count, unsigned* __restrict__ amax) {
    __shared__ float red[4];
    float m = 0.f;
    const size_t nq = count / 4, stride = (size_t)gridDim.x * blockDim.x;
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (((uintptr_t)x & 15) == 0) {
        for (size_t i = i0; i < nq; i += stride) {
            float4 v = ((const float4*)x)[i];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
        for (size_t i = nq * 4 + i0; i < count; i += stride) m = fmaxf(m, fabsf(x[i]));
    } else {
        for (size_t i = i0; i < count; i += stride) m = fmaxf(m, fabsf(x[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        unsigned bits = __float_as_uint(m);
        if (bits > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(amax, bits);
    }
}

extern "C" int xv_amax(void* stream, const float* x, size_t count, uint32_t* amax_accum) {
    XV_REQUIRE(x && amax_accum && count > 0, "amax: bad arguments");
    const int blocks = grid_for((long)(count / 4), 256, 1024);
    hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, count, (unsigned*)amax_accum);
    XV_LAUNCH_CHECK();
    return 0;
}

__device__ __forceinline__ void store_split8(const float (&v)[8], float s, u16* __restrict__ hi, u16* __restrict__ lo) {
    u16 h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_f16(v[j], s, h[j], l[j]);
    *(uint4*)hi = *(const uint4*)h;
    *(uint4*)lo = *(const uint4*)l;
}

// The launch geometry of the two emitters: one thread per 16-byte chunk of a plane row, grid-stride, indexed in 32 bits.
static int emit_grid(const char* who, int rows, int ldp, int* blocks) {
    const long total = (long)rows * (ldp / 8);
    XV_REQUIRE(total < (1L << 31), "%s: tensor too large for 32-bit indexing", who);
    *blocks = grid_for(total, 256, 8192);
    return 0;
}

// chunk i of a plane's [rows][cq] grid of 16-byte chunks: its row, and in `col` its first column
__device__ __forceinline__ long emit_chunk(unsigned i, unsigned cq, int& col) {
    const long r = i / cq;
    col = (int)(i - (unsigned)r * cq) * 8;
    return r;
}

// dst planes [2][rows][ldd] <- src [rows][lds] (columns >= c zero).  8 elements (one 16-byte chunk per plane) per thread;
// VEC: c and lds are multiples of 4 and src is 16-byte aligned, so the 8 inputs are two float4 loads.
template <bool VEC>
__global__ void split_planes_kernel(const float* __restrict__ src, long rows, int c, long lds, u16* __restrict__ dst, long ldd,
                                    long plane_stride, const unsigned* __restrict__ amax) {
    const float s = xv_pow2_scale(*amax);
    const unsigned cq = (unsigned)(ldd / 8), total = (unsigned)rows * cq;      // < 2^31 (checked by the wrapper)
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int col;
        const long r = emit_chunk(i, cq, col);
        float v[8];
        if (VEC) {
            float4 a = col < c ? *(const float4*)(src + r * lds + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 b = col + 4 < c ? *(const float4*)(src + r * lds + col + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (col + j) < c ? src[r * lds + col + j] : 0.f;
        }
        store_split8(v, s, dst + r * ldd + col, dst + plane_stride + r * ldd + col);
    }
}

extern "C" int xv_split_planes(void* stream, const float* src, int rows, int c, int lds, void* planes, int ldp, size_t plane_stride,
                               const uint32_t* amax) {
    XV_REQUIRE(src && planes && amax && rows > 0 && c > 0 && lds >= c, "split_planes: bad arguments");
    XV_REQUIRE(ldp % 8 == 0 && ldp >= c && ((uintptr_t)planes % 16) == 0 && plane_stride % 8 == 0, "split_planes: ldp must be a multiple of 8 and >= c");
    int blocks;
    if (int rc = emit_grid("split_planes", rows, ldp, &blocks)) return rc;
    const bool vec = c % 4 == 0 && lds % 4 == 0 && ((uintptr_t)src % 16) == 0;
    hipLaunchKernelGGL(vec ? split_planes_kernel<true> : split_planes_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src,
                       (long)rows, c, (long)lds, (u16*)planes, (long)ldp, (long)plane_stride, (const unsigned*)amax);
    XV_LAUNCH_CHECK();
    return 0;
}

// planes <- relu?(z*scale + shift)   (BN + ReLU output written directly as the next layer's operand planes)
// n and ldz are multiples of 4 (checked by the wrapper): two float4 loads of z per thread.
__global__ void bn_apply_split_kernel(const float* __restrict__ z, long rows, int n, long ldz, const float* __restrict__ scale,
                                      const float* __restrict__ shift, int relu, const unsigned* __restrict__ amax,
                                      u16* __restrict__ dst, long ldd, long plane_stride, const float* __restrict__ slope) {
    const float s = xv_pow2_scale(*amax);
    const unsigned cq = (unsigned)(ldd / 8), total = (unsigned)rows * cq;      // < 2^31 (checked by the wrapper)
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        int col;
        const long r = emit_chunk(i, cq, col);
        float v[8];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c = col + 4 * q;
            f32x4 y = {0, 0, 0, 0};
            if (c < n) {
                y = *(const f32x4*)(z + r * ldz + c) * *(const f32x4*)(scale + c) + *(const f32x4*)(shift + c);
                if (relu && slope) y = act4(y, *(const f32x4*)(slope + c));      // prelu / leaky ReLU (act context, xv_ew.h)
                else if (relu) y = relu4(y);
            }
            v[4 * q] = y.x; v[4 * q + 1] = y.y; v[4 * q + 2] = y.z; v[4 * q + 3] = y.w;
        }
        store_split8(v, s, dst + r * ldd + col, dst + plane_stride + r * ldd + col);
    }
}

extern "C" int xv_bn_apply_split(void* stream, const float* z, int rows, int n, int ldz, const float* scale, const float* shift, int relu,
                                 const uint32_t* amax, void* planes, int ldp, size_t plane_stride) {
    XV_REQUIRE(rows > 0 && n > 0 && ldz >= n && ldp % 8 == 0 && ldp >= n && plane_stride % 8 == 0, "bn_apply_split: bad shape");
    XV_REQUIRE(n % 4 == 0 && ldz % 4 == 0 && ((uintptr_t)z % 16) == 0, "bn_apply_split: n and ldz must be multiples of 4 (n=%d ldz=%d)", n, ldz);
    int blocks;
    if (int rc = emit_grid("bn_apply_split", rows, ldp, &blocks)) return rc;
    hipLaunchKernelGGL(bn_apply_split_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, z, (long)rows, n, (long)ldz, scale, shift,
                       relu, (const unsigned*)amax, (u16*)planes, (long)ldp, (long)plane_stride, relu ? xv_act_context().slope : nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}
