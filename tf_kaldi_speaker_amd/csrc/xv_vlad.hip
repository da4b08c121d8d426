// GhostVLAD / NetVLAD pooling (model/pooling.py:195-277), fp32:
//   A_t = softmax(x_t W + b) over the K + G clusters        - vlad_softmax_kernel (one wave per frame; the logits come from the dense GEMM)
//   R_k = sum_t A_tk (x_t - c_k), n_k = sum_t A_tk, k < K    - vlad_pool_fwd_kernel (one pass over x per group of 8 clusters)
//   V_k = R_k rsqrt(max(|R_k|^2, 1e-12)) (+ the same over the whole row: vlad_final_l2_norm)   - vlad_norm_fwd_kernel
// and the backward pieces: the normalisations, d A / the value path of d x (one pass over x), the softmax, the centres.
// The residual is summed as A (x - c), not as sum A x - n c: a chunk of frames equal to a centre then gives exactly 0.
// No atomics; every sum has a fixed order, so a call gives the same bits every time.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_pool.h"

namespace {

#define VL_G 8          // clusters per pass: 8 accumulator quads + 8 centre quads per lane
#define VL_EPS 1e-12f   // tf.nn.l2_normalize's epsilon (on the squared norm)

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float hsum4(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// a[r][j] = softmax_j(logits[r][j]), j < kg <= 64: lane j holds cluster j, the columns kg .. ld of the logits (GEMM padding) are never read
__global__ __launch_bounds__(256) void vlad_softmax_kernel(const float* __restrict__ logits, int rows, int kg, int ld, float* __restrict__ a) {
    XV_EW_PRIORITY();
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bool on = lane < kg;
    const float v = on ? logits[(long)row * ld + lane] : -INFINITY;
    const float m = wave_max_f(v);
    const float e = on ? expf(v - m) : 0.f;
    const float z = wave_sum(e);
    if (on) a[(long)row * kg + lane] = e / z;
}

// dl[r][j] = a (da - sum_j a da) for j < kg, 0 for kg <= j < ld (the GEMMs behind it read whole rows)
__global__ __launch_bounds__(256) void vlad_softmax_bwd_kernel(const float* __restrict__ a, const float* __restrict__ da, int rows, int kg, int ld,
                                                               float* __restrict__ dl) {
    XV_EW_PRIORITY();
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bool on = lane < kg;
    const float w = on ? a[(long)row * kg + lane] : 0.f;
    const float g = on ? da[(long)row * kg + lane] : 0.f;
    const float z = wave_sum(w * g);
    if (lane < ld) dl[(long)row * ld + lane] = on ? w * (g - z) : 0.f;
}

// block = 64 column quads x 4 frame lanes (the layout of stat_pool_fwd_kernel), grid = (column blocks, chunks, cluster groups).
// Each lane keeps VL_G residual quads and the VL_G centre quads; the frame weights of a wave's frame are wave-uniform.
__global__ __launch_bounds__(256) void vlad_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ cen,
                                                            int T, int C, int K, int KG, const int* __restrict__ flen, int shrink,
                                                            float* __restrict__ r, float* __restrict__ n) {
    XV_EW_PRIORITY();
    __shared__ f32x4 s_acc[3][VL_G][64];
    __shared__ float s_n[4][VL_G];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int col = (blockIdx.x * 64 + lane) * 4;
    const int b = blockIdx.y, k0 = blockIdx.z * VL_G;
    const bool cv = col < C;
    const float* xp = x + (long)b * T * C + (cv ? col : 0);
    const float* ap = a + (long)b * T * KG;
    if (flen) T = max(1, min(T, flen[b] - shrink));      // batched extraction: the rows behind are padding (xv_stat_pool_forward_bn_ex)
    int kk[VL_G];
    f32x4 cq[VL_G], acc[VL_G];
    float nn[VL_G];
#pragma unroll
    for (int j = 0; j < VL_G; ++j) {
        kk[j] = min(k0 + j, K - 1);      // (clamped: a group's unused slots repeat the last cluster and are not written)
        cq[j] = *(const f32x4*)(cen + (long)kk[j] * C + (cv ? col : 0));
        acc[j] = f32x4{0, 0, 0, 0};
        nn[j] = 0.f;
    }
    int t = wave;
    for (; t + 12 < T; t += 16) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const f32x4*)(xp + (long)(t + 4 * u) * C);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* at = ap + (long)(t + 4 * u) * KG;
#pragma unroll
            for (int j = 0; j < VL_G; ++j) {
                const float w = at[kk[j]];
                acc[j] += (v[u] - cq[j]) * w;
                nn[j] += w;
            }
        }
    }
    for (; t < T; t += 4) {
        const f32x4 v = *(const f32x4*)(xp + (long)t * C);
        const float* at = ap + (long)t * KG;
#pragma unroll
        for (int j = 0; j < VL_G; ++j) {
            const float w = at[kk[j]];
            acc[j] += (v - cq[j]) * w;
            nn[j] += w;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < VL_G; ++j) s_acc[wave - 1][j][lane] = acc[j];
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VL_G; ++j) s_n[wave][j] = nn[j];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int j = 0; j < VL_G; ++j) {
        if (k0 + j >= K) break;
        if (cv) *(f32x4*)(r + ((long)b * K + k0 + j) * C + col) = ((acc[j] + s_acc[0][j][lane]) + s_acc[1][j][lane]) + s_acc[2][j][lane];
        if (blockIdx.x == 0 && lane == 0) n[(long)b * K + k0 + j] = ((s_n[0][j] + s_n[1][j]) + s_n[2][j]) + s_n[3][j];
    }
}

// One workgroup per chunk, a wave per cluster: V_k = R_k rsqrt(max(|R_k|^2, eps)); final: the K*C row once more the same way
__global__ __launch_bounds__(256) void vlad_norm_fwd_kernel(const float* __restrict__ r, int K, int C, int final_norm, float* __restrict__ out) {
    XV_EW_PRIORITY();
    __shared__ float s_inv[64], s_vs[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nq = C >> 2;
    const float* rb = r + (long)blockIdx.x * K * C;
    float* ob = out + (long)blockIdx.x * K * C;
    for (int k = wave; k < K; k += 4) {
        float ss = 0.f;
        for (int q = lane; q < nq; q += 64) { const f32x4 v = *(const f32x4*)(rb + (long)k * C + 4 * q); ss += hsum4(v * v); }
        ss = wave_sum(ss);
        const float inv = rsqrtf(fmaxf(ss, VL_EPS));
        if (lane == 0) { s_inv[k] = inv; s_vs[k] = ss * inv * inv; }
    }
    __syncthreads();
    float f = 1.f;
    if (final_norm) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += s_vs[k];
        f = rsqrtf(fmaxf(s, VL_EPS));
    }
    for (int k = wave; k < K; k += 4) {
        const float inv = s_inv[k];
        for (int q = lane; q < nq; q += 64) *(f32x4*)(ob + (long)k * C + 4 * q) = *(const f32x4*)(rb + (long)k * C + 4 * q) * inv * f;
    }
}

// d R from d out.  Final normalisation y = V f, f = rsqrt(max(s, eps)), s = sum |V_k|^2:  dV = f dy - [s >= eps] f^3 (V.dy) V;
// per cluster V = R inv:  dR = inv dV - [|R|^2 >= eps] inv^3 (R.dV) R.  A clamped norm passes the gradient through the constant 1e6
// (the maximum()'s other branch has no gradient), so a zero residual gives finite values.
__global__ __launch_bounds__(256) void vlad_norm_bwd_kernel(const float* __restrict__ r, const float* __restrict__ dout, int K, int C, int final_norm,
                                                            float* __restrict__ dr) {
    XV_EW_PRIORITY();
    __shared__ float s_ss[64], s_p[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nq = C >> 2;
    const float* rb = r + (long)blockIdx.x * K * C;
    const float* gb = dout + (long)blockIdx.x * K * C;
    float* ob = dr + (long)blockIdx.x * K * C;
    for (int k = wave; k < K; k += 4) {
        float ss = 0.f, p = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const f32x4 v = *(const f32x4*)(rb + (long)k * C + 4 * q), g = *(const f32x4*)(gb + (long)k * C + 4 * q);
            ss += hsum4(v * v);
            p += hsum4(v * g);
        }
        ss = wave_sum(ss);
        p = wave_sum(p);
        if (lane == 0) { s_ss[k] = ss; s_p[k] = p; }
    }
    __syncthreads();
    float f = 1.f, cf = 0.f;
    if (final_norm) {
        float s = 0.f, d = 0.f;      // s = sum |V_k|^2, d = V . dy
        for (int k = 0; k < K; ++k) {
            const float inv = rsqrtf(fmaxf(s_ss[k], VL_EPS));
            s += s_ss[k] * inv * inv;
            d += s_p[k] * inv;
        }
        f = rsqrtf(fmaxf(s, VL_EPS));
        cf = s >= VL_EPS ? f * f * f * d : 0.f;
    }
    for (int k = wave; k < K; k += 4) {
        const float ss = s_ss[k], inv = rsqrtf(fmaxf(ss, VL_EPS));
        // dV = f dy - cf inv R;  R . dV = f p - cf inv ss
        const float qk = f * s_p[k] - cf * inv * ss;
        const float ck = ss >= VL_EPS ? inv * inv * inv * qk : 0.f;
        const float gy = inv * f, gr = inv * inv * cf + ck;
        for (int q = lane; q < nq; q += 64) {
            const f32x4 v = *(const f32x4*)(rb + (long)k * C + 4 * q), g = *(const f32x4*)(gb + (long)k * C + 4 * q);
            *(f32x4*)(ob + (long)k * C + 4 * q) = g * gy - v * gr;
        }
    }
}

// One pass over x: a wave takes four consecutive frames of a chunk (they share every d R / centre load) and, per group of VL_G clusters,
//   da[t][k] = (x_t - c_k) . dR_k   (wave-reduced dots)      dx[t] = sum_k a[t][k] dR_k   (the value path of d x)
// K <= VL_G is one group: x is read once.  A further group reads its rows again and adds to the dx rows it wrote itself.
__global__ __launch_bounds__(256) void vlad_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ cen,
                                                            const float* __restrict__ dr, int B, int T, int C, int K, int KG,
                                                            float* __restrict__ da, float* __restrict__ dx) {
    XV_EW_PRIORITY();
    const int lane = threadIdx.x & 63;
    const int wg = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int rbpc = (T + 3) >> 2;
    const int b = wg / rbpc;
    if (b >= B) return;
    const int t0 = (wg - b * rbpc) * 4;
    const int nq = C >> 2;
    long row[4];
    bool rv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { rv[i] = t0 + i < T; row[i] = (long)b * T + min(t0 + i, T - 1); }
    const float* drb = dr + (long)b * K * C;
    for (int k0 = 0; k0 < K; k0 += VL_G) {
        int kk[VL_G];
        float aw[4][VL_G], dot[4][VL_G];
#pragma unroll
        for (int j = 0; j < VL_G; ++j) {
            kk[j] = min(k0 + j, K - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) { aw[i][j] = k0 + j < K ? a[row[i] * KG + kk[j]] : 0.f; dot[i][j] = 0.f; }
        }
        for (int q0 = 0; q0 < nq; q0 += 64) {
            const bool ok = q0 + lane < nq;
            const int c4 = 4 * min(q0 + lane, nq - 1);
            f32x4 xv[4], dxq[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = *(const f32x4*)(x + row[i] * C + c4);
#pragma unroll
            for (int i = 0; i < 4; ++i) dxq[i] = k0 > 0 ? *(const f32x4*)(dx + row[i] * C + c4) : f32x4{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < VL_G; ++j) {
                const f32x4 dq = *(const f32x4*)(drb + (long)kk[j] * C + c4), cq = *(const f32x4*)(cen + (long)kk[j] * C + c4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = hsum4((xv[i] - cq) * dq);
                    dot[i][j] += ok ? d : 0.f;
                    dxq[i] += dq * aw[i][j];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ok && rv[i]) *(f32x4*)(dx + row[i] * C + c4) = dxq[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < VL_G; ++j) {
                const float d = wave_sum(dot[i][j]);
                if (lane == 0 && rv[i] && k0 + j < K) da[row[i] * KG + k0 + j] = d;
            }
        }
    }
    // ghost clusters take part in the softmax only
    if (lane >= K && lane < KG) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (rv[i]) da[row[i] * KG + lane] = 0.f;
    }
}

// dc[k] = -sum_b n[b][k] dR[b][k] for k < K, 0 for the ghosts; + l2 * c[k] (the regulariser covers every centre).  block = 16 column quads x
// 16 chunk lanes, grid = (column blocks, clusters): a lane adds chunks lane, lane + 16, ... in order, the 16 lanes are added in order
// (one thread per cluster column over all chunks took 62 us at 128 chunks: 3 750 threads, 128 dependent loads each)
#define VL_CB 16
__global__ __launch_bounds__(256) void vlad_centers_bwd_kernel(const float* __restrict__ n, const float* __restrict__ dr, const float* __restrict__ cen,
                                                               int B, int K, int KG, int C, float l2, float* __restrict__ dc) {
    XV_EW_PRIORITY();
    __shared__ f32x4 red[VL_CB][16];
    const int qx = threadIdx.x & 15, bl = threadIdx.x >> 4;
    const int k = blockIdx.y, c4 = 4 * (blockIdx.x * 16 + qx);
    const bool cv = c4 < C;
    f32x4 s = {0, 0, 0, 0};
    if (cv && k < K)
        for (int b = bl; b < B; b += VL_CB) s += *(const f32x4*)(dr + ((long)b * K + k) * C + c4) * n[(long)b * K + k];
    red[bl][qx] = s;
    __syncthreads();
    if (bl != 0 || !cv) return;
    for (int j = 1; j < VL_CB; ++j) s += red[j][qx];
    *(f32x4*)(dc + (long)k * C + c4) = *(const f32x4*)(cen + (long)k * C + c4) * l2 - s;
}

// dst[r][j] = j < cols ? src[r][j] : 0 for j < ldd: a matrix between two row pitches (W and d W between their [C][K + G] variables and the
// GEMM operands on whole column quads), as a launch like its neighbours (no copy engine, no packet of the runtime's 2-D copy path).
__global__ __launch_bounds__(256) void vlad_repitch_kernel(const float* __restrict__ src, int rows, int cols, int lds, float* __restrict__ dst, int ldd) {
    XV_EW_FILLER();
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * ldd) return;
    const int r = (int)(i / ldd), j = (int)(i - (long)r * ldd);
    dst[i] = j < cols ? src[(long)r * lds + j] : 0.f;
}

bool vl_shape_ok(int c, int k, int kg) { return c > 0 && c % 4 == 0 && k >= 1 && kg >= k && kg <= 64; }

}  // namespace

extern "C" int xv_vlad_repitch(void* stream, const float* src, int rows, int cols, int lds, float* dst, int ldd) {
    XV_REQUIRE(src && dst && rows > 0 && cols > 0 && lds > 0 && ldd > 0 && (cols <= lds || rows == 1) && (long)rows * ldd < (1L << 31),
               "vlad_repitch: bad arguments (%d x %d, pitches %d -> %d)", rows, cols, lds, ldd);
    hipLaunchKernelGGL(vlad_repitch_kernel, dim3(xv_cdiv((long)rows * ldd, 256)), dim3(256), 0, (hipStream_t)stream, src, rows, cols, lds, dst, ldd);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_softmax(void* stream, const float* logits, int rows, int kg, int ld, float* a) {
    XV_REQUIRE(logits && a && rows > 0 && kg >= 1 && kg <= 64 && ld >= kg, "vlad_softmax: bad arguments (1 <= clusters <= 64 <= row pitch; got %d, %d)", kg, ld);
    hipLaunchKernelGGL(vlad_softmax_kernel, dim3(xv_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, logits, rows, kg, ld, a);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_softmax_backward(void* stream, const float* a, const float* da, int rows, int kg, int ld, float* dl) {
    XV_REQUIRE(a && da && dl && rows > 0 && kg >= 1 && kg <= 64 && ld >= kg && ld <= 64, "vlad_softmax_backward: bad arguments (clusters %d, row pitch %d)", kg, ld);
    hipLaunchKernelGGL(vlad_softmax_bwd_kernel, dim3(xv_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, a, da, rows, kg, ld, dl);
    XV_LAUNCH_CHECK();
    return 0;
}

int xv_vlad_pool_forward_ex(hipStream_t s, const float* x, const float* a, const float* centers, int b, int t, int c, int k, int kg,
                            const int32_t* frames, int shrink, float* r, float* n) {
    XV_REQUIRE(x && a && centers && r && n && b > 0 && t > 0 && vl_shape_ok(c, k, kg),
               "vlad_pool_forward: bad arguments (c=%d must be a multiple of 4, 1 <= centers %d <= clusters %d <= 64)", c, k, kg);
    hipLaunchKernelGGL(vlad_pool_fwd_kernel, dim3(xv_cdiv(c / 4, 64), b, xv_cdiv(k, VL_G)), dim3(256), 0, s, x, a, centers, t, c, k, kg,
                       (const int*)frames, shrink, r, n);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_pool_forward(void* stream, const float* x, const float* a, const float* centers, int b, int t, int c, int k, int kg,
                                    const int32_t* frames, int shrink, float* r, float* n) {
    return xv_vlad_pool_forward_ex((hipStream_t)stream, x, a, centers, b, t, c, k, kg, frames, shrink, r, n);
}

extern "C" int xv_vlad_normalize_forward(void* stream, const float* r, int b, int k, int c, int final_norm, float* out) {
    XV_REQUIRE(r && out && b > 0 && vl_shape_ok(c, k, k), "vlad_normalize_forward: bad arguments (c=%d must be a multiple of 4, 1 <= centers %d <= 64)", c, k);
    hipLaunchKernelGGL(vlad_norm_fwd_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, r, k, c, final_norm, out);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_normalize_backward(void* stream, const float* r, const float* dout, int b, int k, int c, int final_norm, float* dr) {
    XV_REQUIRE(r && dout && dr && b > 0 && vl_shape_ok(c, k, k), "vlad_normalize_backward: bad arguments (c=%d must be a multiple of 4, 1 <= centers %d <= 64)", c, k);
    hipLaunchKernelGGL(vlad_norm_bwd_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, r, dout, k, c, final_norm, dr);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_pool_backward(void* stream, const float* x, const float* a, const float* centers, const float* dr, int b, int t, int c, int k,
                                     int kg, float* da, float* dx) {
    XV_REQUIRE(x && a && centers && dr && da && dx && b > 0 && t > 0 && vl_shape_ok(c, k, kg),
               "vlad_pool_backward: bad arguments (c=%d must be a multiple of 4, 1 <= centers %d <= clusters %d <= 64)", c, k, kg);
    const long waves = (long)b * ((t + 3) / 4);
    hipLaunchKernelGGL(vlad_pool_bwd_kernel, dim3(xv_cdiv(waves, 4)), dim3(256), 0, (hipStream_t)stream, x, a, centers, dr, b, t, c, k, kg, da, dx);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_vlad_centers_backward(void* stream, const float* n, const float* dr, const float* centers, int b, int k, int kg, int c, float l2,
                                        float* dc) {
    XV_REQUIRE(n && dr && centers && dc && b > 0 && vl_shape_ok(c, k, kg),
               "vlad_centers_backward: bad arguments (c=%d must be a multiple of 4, 1 <= centers %d <= clusters %d <= 64)", c, k, kg);
    hipLaunchKernelGGL(vlad_centers_bwd_kernel, dim3(xv_cdiv(c / 4, 16), kg), dim3(256), 0, (hipStream_t)stream, n, dr, centers, b, k, kg, c,
                       l2, dc);
    XV_LAUNCH_CHECK();
    return 0;
}
