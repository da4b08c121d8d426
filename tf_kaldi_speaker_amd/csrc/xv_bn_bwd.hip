// BatchNorm (+ activation) backward of the frame-level tensors: the two reductions (plain pass, pooled pass, closed form from the pooled
// statistics, or partials left by a GEMM epilogue), their finalisation, and dz in the fp32 and the split-precision layout.  The upstream
// gradient is a tensor in memory or the statistics-pooling backward evaluated on the fly.  Threads run along channels (16 B per lane),
// reductions over rows are per-thread serial + LDS combine in a fixed order; no atomics on any path that feeds a gradient.  gfx950 only.
#include <algorithm>

#include "xv_common.h"
#include "xv_ew.h"
#include "xv_bn.h"
#include "xv_epilogue.h"

// The launch plan of the backward (bn_bwd_plan below; xv_debug_bn_bwd_plan reports it).  Reduction forms, the template flags of the pooled
// pass, apply forms:
enum { XV_BNB_CLOSED = 0, XV_BNB_POOLED = 1, XV_BNB_PLAIN = 2, XV_BNB_EXTERNAL = 3 };
enum { XV_BNB_ATT = 1, XV_BNB_HS = 2, XV_BNB_RELU = 4 };
enum { XV_BNB_DENSE = 0, XV_BNB_STRIP = 1, XV_BNB_SPLIT = 2 };
struct BnBwdPlan { int reduce, flags, nstat, chunks, apply; };

// Upstream gradient of a layer whose output feeds statistics pooling directly (tdnn5): instead of reading a
// materialised d(activation), the BN backward evaluates the pooling backward (pooling.py:9-34) on the fly from the
// pooled statistics [b][mean | std] and their gradient:  da = dmean/T + dstd/(T*std) * (a - mean),  a = relu?(z*scale+shift).
struct PoolGrad { const float* out; const float* dout; int t; const float* w; const float* wpos; const float* amax; };   // w: per-frame attention weights or null (1/t)
// wpos [b][n] (optional): the share of each chunk's frame weights that sits on frames with an active ReLU, written by the pooling forward -
// with it the BatchNorm backward's two reductions have a closed form per (chunk, channel) and the pass over z is not needed (bn_bwd_pooled_stats_kernel).
// amax [b][n] (optional): each chunk's largest activation - bounds |d a| for the split-precision dz scale

// The pooled statistics of chunk b at one channel quad, in the form the per-element formula needs: they change only when
// the row loop crosses into the next chunk, so the kernels reload them there instead of once per element (4 vector loads,
// 4 divisions and an integer division by T per 16 bytes of z before).
struct PoolCoef { f32x4 mean, dm, q; };      // q = dstd / std (0 where the forward clamped the variance)
__device__ __forceinline__ PoolCoef pool_coef(const PoolGrad& pg, int b, int n, int col) {
    const float sd_eps = 1e-6f;      // sqrt(1e-12): the forward clamps the variance there (pooling.py:28-29)
    const float* o = pg.out + (long)b * 2 * n;
    const float* g = pg.dout + (long)b * 2 * n;
    PoolCoef pc;
    pc.mean = *(const f32x4*)(o + col);
    pc.dm = *(const f32x4*)(g + col);
    const f32x4 sd = *(const f32x4*)(o + n + col), ds = *(const f32x4*)(g + n + col);
    pc.q.x = sd.x <= sd_eps ? 0.f : ds.x / sd.x; pc.q.y = sd.y <= sd_eps ? 0.f : ds.y / sd.y;
    pc.q.z = sd.z <= sd_eps ? 0.f : ds.z / sd.z; pc.q.w = sd.w <= sd_eps ? 0.f : ds.w / sd.w;
    return pc;
}
// da = dmean * w + (dstd / std * w) * (a - mean), w = 1/T or the frame's attention weight (pooling.py:148-155)
__device__ __forceinline__ f32x4 pool_grad(const PoolCoef& pc, float invT, f32x4 a) {
    return pc.dm * invT + (pc.q * invT) * (a - pc.mean);
}
__device__ __forceinline__ float pool_frame_weight(const PoolGrad& pg, long row) { return pg.w ? pg.w[row] : 1.f / (float)pg.t; }

// masked upstream gradient of one channel quad: the gradient `dd` read from memory, or the pooling backward on the fly (frame weight w),
// zeroed (scaled by the slope) where the activation was off.  sl / hs: the activation's negative-side slope of this channel quad and
// whether there is one (act context).
__device__ __forceinline__ f32x4 upstream_grad(f32x4 dd, f32x4 zz, f32x4 sc, f32x4 sh, int relu, f32x4 sl, bool hs) {
    return relu ? mask_grad4(dd, zz * sc + sh, sl, hs) : dd;
}
__device__ __forceinline__ f32x4 upstream_grad_pooled(const PoolCoef& pc, float w, f32x4 zz, f32x4 sc, f32x4 sh, int relu, f32x4 sl, bool hs) {
    const f32x4 y = zz * sc + sh;
    f32x4 a = y;
    if (relu) a = hs ? act4(a, sl) : relu4(a);
    const f32x4 dd = pool_grad(pc, w, a);
    return relu ? mask_grad4(dd, y, sl, hs) : dd;
}

// The end of both reduction kernels: a block's 64 channel quads x 4 row lanes of sums (s1, s2, s4) and maxima (s3) are combined over the
// row lanes in the fixed order (r0 + r1) + (r2 + r3) and stored as the partials [nstat][n] of block blockIdx.y (barrier inside).
__device__ __forceinline__ void bn_bwd_store_partials(f32x4 (*red)[4][64], f32x4 s1, f32x4 s2, f32x4 s3, f32x4 s4, int rl, int qx, int col,
                                                      int n, int nstat, float* __restrict__ part) {
    red[0][rl][qx] = s1; red[1][rl][qx] = s2; red[2][rl][qx] = s3; red[3][rl][qx] = s4;
    __syncthreads();
    if (rl == 0 && col < n) {
        const f32x4 t3 = max4(max4(red[2][0][qx], red[2][1][qx]), max4(red[2][2][qx], red[2][3][qx]));
        float* o = part + (long)blockIdx.y * nstat * n + col;
        *(f32x4*)(o) = (red[0][0][qx] + red[0][1][qx]) + (red[0][2][qx] + red[0][3][qx]);
        *(f32x4*)(o + n) = (red[1][0][qx] + red[1][1][qx]) + (red[1][2][qx] + red[1][3][qx]);
        *(f32x4*)(o + 2 * n) = t3;
        if (nstat == 4) *(f32x4*)(o + 3 * n) = (red[3][0][qx] + red[3][1][qx]) + (red[3][2][qx] + red[3][3][qx]);
    }
}

// upper bound of |dz| = |gamma*invstd| * |dy - c1 - xhat*c2| of one channel over the batch (the split-precision operand scale): s3 bounds
// |dy|, [zmin, zmax] the range of z
__device__ __forceinline__ float bn_dz_bound(float gamma, float invstd, float mean, float zmin, float zmax, float s3, float c1, float c2) {
    const float xh = fmaxf(fabsf(zmax - mean), fabsf(zmin - mean)) * invstd;
    return fabsf(gamma * invstd) * (s3 + fabsf(c1) + xh * fabsf(c2)) * 1.0001f;
}

// Backward pass 1: per (64-row chunk, 256-column block) partial sums of dy and dy*xhat (upstream gradient d a in memory; the pooled
// form is bn_bwd_reduce_pooled_kernel below).
// block = 256 threads = 64 column-quads x 4 row lanes.
#define BB_ROWS 64
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ da, const float* __restrict__ z, int rows,
                                                            int n, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int relu,
                                                            float* __restrict__ part /* [chunks][nstat][n]: sum dy, sum dy*xhat, max |dy| (, sum d act*min(y,0)) */,
                                                            const float* __restrict__ slope, int nstat) {
    XV_EW_PRIORITY();
    __shared__ f32x4 red[4][4][64];
    const int qx = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + qx) * 4;
    const int r0 = blockIdx.y * BB_ROWS, r1 = min(rows, r0 + BB_ROWS);
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0}, s3 = {0, 0, 0, 0}, s4 = {0, 0, 0, 0};
    const bool hs = slope != nullptr, want4 = nstat == 4;
    if (col < n) {
        f32x4 mu = *(const f32x4*)(mean + col), is = *(const f32x4*)(invstd + col);
        f32x4 sc = *(const f32x4*)(scale + col), sh = *(const f32x4*)(shift + col);
        f32x4 sl = {0, 0, 0, 0};
        if (hs) sl = *(const f32x4*)(slope + col);
        // one row per trip: [measured] four rows' loads issued together make this form slower inside the step (42 -> 46 us; its 50 MB
        // tensors sit in the Infinity Cache)
        for (int r = r0 + rl; r < r1; r += 4) {
            const f32x4 zz = *(const f32x4*)(z + (long)r * n + col);
            // (the prelu term d act * min(y, 0) is formed here, from the unmasked gradient: handing upstream_grad a pointer for it put
            // the value in scratch memory - 32 bytes per lane, written and re-read once per row - in the kernel the data-gradient chain waits for)
            const f32x4 raw = *(const f32x4*)(da + (long)r * n + col);
            if (want4 && relu) s4 += raw * neg4(zz * sc + sh);
            f32x4 dd = upstream_grad(raw, zz, sc, sh, relu, sl, hs);
            f32x4 xh = (zz - mu) * is;
            s1 += dd;
            s2 += dd * xh;
            s3 = absmax4(s3, dd);
        }
    }
    bn_bwd_store_partials(red, s1, s2, s3, s4, rl, qx, col, n, nstat, part);
}

// The POOLED reductions as a kernel of their own (prelu / lrelu / attention pooling: the cases without a closed form).  A workgroup stays
// inside ONE chunk of the batch (grid.y = chunk x row block), so the pooled statistics, their four divisions and 1/T are loaded once per
// thread, the row loop has no chunk-crossing branch and keeps eight 16-byte loads of z in flight per lane; rows beyond the block carry a
// frame weight of zero (every summand of theirs is 0) instead of a predicate.  [measured, round 2, 143 MB of z at S1] the generic kernel above
// needed 52.7 us (86 branches, a vmcnt(0) per row) where the pooling forward reads the same bytes in 27.5 us.
#define BBP_ROWS 64
#define BBP_FLIGHT 8
template <bool RELU, bool HS, bool ATT>
__global__ __launch_bounds__(256) void bn_bwd_reduce_pooled_kernel(PoolGrad pg, const float* __restrict__ z, int n, int nsub, int rows_per,
                                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   float* __restrict__ part /* [chunks * nsub][nstat][n] */,
                                                                   const float* __restrict__ slope, int nstat) {
    XV_EW_PRIORITY();
    __shared__ f32x4 red[4][4][64];
    const int qx = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + qx) * 4;
    const int b = blockIdx.y / nsub, jb = blockIdx.y - b * nsub;
    const int r0 = b * pg.t + jb * rows_per, r1 = min((b + 1) * pg.t, r0 + rows_per);
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0}, s3 = {0, 0, 0, 0}, s4 = {0, 0, 0, 0};
    if (col < n && r0 < r1) {
        const f32x4 mu = *(const f32x4*)(mean + col), is = *(const f32x4*)(invstd + col);
        const f32x4 sc = *(const f32x4*)(scale + col), sh = *(const f32x4*)(shift + col);
        f32x4 sl = {0, 0, 0, 0};
        if (HS) sl = *(const f32x4*)(slope + col);
        const PoolCoef pc = pool_coef(pg, b, n, col);
        const float w_uniform = 1.f / (float)pg.t;
        const float* __restrict__ zc = z + col;
        for (int rb = r0 + rl; rb < r1; rb += 4 * BBP_FLIGHT) {
            f32x4 zq[BBP_FLIGHT];
            float wq[BBP_FLIGHT];
#pragma unroll
            for (int j = 0; j < BBP_FLIGHT; ++j) {
                const int r = min(rb + 4 * j, r1 - 1);
                zq[j] = *(const f32x4*)(zc + (long)r * n);
                wq[j] = ATT ? pg.w[r] : w_uniform;
            }
#pragma unroll
            for (int j = 0; j < BBP_FLIGHT; ++j) {
                const float w = rb + 4 * j < r1 ? wq[j] : 0.f;
                const f32x4 y = zq[j] * sc + sh;
                f32x4 a = y;
                if (RELU) a = HS ? act4(a, sl) : relu4(a);
                f32x4 dd = pool_grad(pc, w, a);
                if (RELU) {
                    if (HS) s4 += dd * neg4(y);
                    dd = mask_grad4(dd, y, sl, HS);
                }
                const f32x4 xh = (zq[j] - mu) * is;
                s1 += dd;
                s2 += dd * xh;
                s3 = absmax4(s3, dd);
            }
        }
    }
    bn_bwd_store_partials(red, s1, s2, s3, s4, rl, qx, col, n, nstat, part);
}

// the POOLED reductions of (z, pooled statistics) into part [bn_bwd_pooled_chunks][nstat][n]; flags: the instantiation (bn_bwd_plan)
static void launch_bn_bwd_reduce_pooled(hipStream_t s, const PoolGrad& pg, const float* z, int rows, int n, const float* mean, const float* invstd,
                                        const float* scale, const float* shift, int flags, float* part, const float* slope, int nstat) {
    const int nb = rows / pg.t, nsub = xv_cdiv(pg.t, BBP_ROWS), rows_per = xv_cdiv(pg.t, nsub);
    const dim3 grid(xv_cdiv(n / 4, 64), nb * nsub), block(256);
#define XV_BBP(R, H, A) hipLaunchKernelGGL((bn_bwd_reduce_pooled_kernel<R, H, A>), grid, block, 0, s, pg, z, n, nsub, rows_per, mean, invstd, scale, shift, part, slope, nstat)
    switch (flags) {
    case XV_BNB_ATT: XV_BBP(false, false, true); break;
    case 0: XV_BBP(false, false, false); break;
    case XV_BNB_RELU | XV_BNB_HS | XV_BNB_ATT: XV_BBP(true, true, true); break;
    case XV_BNB_RELU | XV_BNB_HS: XV_BBP(true, true, false); break;
    case XV_BNB_RELU | XV_BNB_ATT: XV_BBP(true, false, true); break;
    default: XV_BBP(true, false, false); break;
    }
#undef XV_BBP
}
static int bn_bwd_pooled_chunks(int rows, int t) { return (rows / t) * xv_cdiv(t, BBP_ROWS); }

// block = 256 threads = 8 channels x 32 chunk lanes, fixed-order combine
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ part, int chunks, int n, int rows,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ coef /* [2][n] */,
                                                              const float* __restrict__ gamma, const float* __restrict__ invstd,
                                                              float* __restrict__ dbias, const float* __restrict__ mean,
                                                              const float* __restrict__ zmin, const float* __restrict__ zmax,
                                                              unsigned* __restrict__ dz_amax, int nstat, float* __restrict__ dalpha) {
    XV_EW_PRIORITY();
    __shared__ float r1[FIN_LANES][FIN_CH], r2[FIN_LANES][FIN_CH], r3[FIN_LANES][FIN_CH], r4[FIN_LANES][FIN_CH];
    const int cx = threadIdx.x & (FIN_CH - 1), cl = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + cx;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    if (c < n)
        for (int k0 = cl; k0 < chunks; k0 += FIN_LANES * FIN_BATCH) {      // FIN_BATCH chunks' loads in flight, summed in chunk order
            float p1[FIN_BATCH], p2[FIN_BATCH], p3[FIN_BATCH], p4[FIN_BATCH];
#pragma unroll
            for (int u = 0; u < FIN_BATCH; ++u) {
                const long k = min(k0 + u * FIN_LANES, chunks - 1);
                p1[u] = part[(k * nstat + 0) * n + c];
                p2[u] = part[(k * nstat + 1) * n + c];
                p3[u] = part[(k * nstat + 2) * n + c];
                p4[u] = nstat == 4 ? part[(k * nstat + 3) * n + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < FIN_BATCH; ++u) {
                if (k0 + u * FIN_LANES >= chunks) break;
                s1 += p1[u];
                s2 += p2[u];
                s3 = fmaxf(s3, p3[u]);
                s4 += p4[u];
            }
        }
    r1[cl][cx] = s1; r2[cl][cx] = s2; r3[cl][cx] = s3; r4[cl][cx] = s4;
    __syncthreads();
    if (cl != 0 || c >= n) return;
    s1 = 0.f; s2 = 0.f; s3 = 0.f; s4 = 0.f;
#pragma unroll
    for (int k = 0; k < FIN_LANES; ++k) { s1 += r1[k][cx]; s2 += r2[k][cx]; s3 = fmaxf(s3, r3[k][cx]); s4 += r4[k][cx]; }
    dbeta[c] = s1;
    dgamma[c] = s2;
    if (dalpha) dalpha[c] = s4;
    const float c1 = s1 / (float)rows;
    coef[c] = c1;
    coef[n + c] = s2 / (float)rows;
    if (dbias) dbias[c] = gamma[c] * invstd[c] * (s1 - c1 * (float)rows);   // == sum(dz) up to rounding: 0 + noise
    if (dz_amax) atomicMax(dz_amax, __float_as_uint(bn_dz_bound(gamma[c], invstd[c], mean[c], zmin[c], zmax[c], s3, c1, s2 / (float)rows)));
}

// Backward pass 2: dz = gamma*invstd*(dy - c1 - xhat*c2) into the segment-padded layout (fp32).
// Thread = one channel quad (16 B) x a strip of rows, block = 64 quads x 4 row lanes over BAF_ROWS padded rows: the seven
// per-channel parameter vectors are loaded once per thread and the pooled statistics once per chunk (the element-per-thread
// form reloaded both - and divided - for every 16 bytes of z: 115 us for tdnn5's 143 MB at S1).
#define BAF_ROWS 32
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ da, PoolGrad pg, const float* __restrict__ z, int segs,
                                                           int t, int n, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ coef, int relu, int pad,
                                                           float* __restrict__ dz, const float* __restrict__ slope, int ldz /* rows of z and dz */) {
    XV_EW_PRIORITY();
    const int tp = t + 2 * pad;
    const int col = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int rl = threadIdx.x >> 6;
    if (col >= n) return;
    const int total_rows = segs * tp;
    const int r0 = blockIdx.y * BAF_ROWS, r1 = min(total_rows, r0 + BAF_ROWS);
    const f32x4 mu = *(const f32x4*)(mean + col), is = *(const f32x4*)(invstd + col);
    const f32x4 sc = *(const f32x4*)(scale + col), sh = *(const f32x4*)(shift + col);
    const f32x4 c1 = *(const f32x4*)(coef + col), c2 = *(const f32x4*)(coef + n + col);
    const f32x4 g_is = *(const f32x4*)(gamma + col) * is;
    const bool hs = slope != nullptr;
    f32x4 sl = {0, 0, 0, 0};
    if (hs) sl = *(const f32x4*)(slope + col);
    int seg = r0 / tp, u = r0 - seg * tp;          // padded row r0 -> (segment, frame + pad)
    u += rl;
    while (u >= tp) { u -= tp; ++seg; }
    PoolCoef pc = {};
    int b_end = 0;                                 // first row beyond the chunk whose statistics are in pc
    float invT = 0.f;
    for (int dr = r0 + rl; dr < r1; dr += 4) {
        f32x4 out = {0, 0, 0, 0};
        const int f = u - pad;
        if (f >= 0 && f < t) {
            const long r = (long)seg * t + f;
            if (POOLED) {
                if (r >= b_end) {
                    const int pb = (int)r / pg.t;
                    b_end = (pb + 1) * pg.t;
                    pc = pool_coef(pg, pb, n, col);
                }
                invT = pool_frame_weight(pg, r);
            }
            const f32x4 zz = *(const f32x4*)(z + r * ldz + col);
            const f32x4 dd = POOLED ? upstream_grad_pooled(pc, invT, zz, sc, sh, relu, sl, hs)
                                    : upstream_grad(*(const f32x4*)(da + r * n + col), zz, sc, sh, relu, sl, hs);
            const f32x4 xh = (zz - mu) * is;
            out = g_is * (dd - c1 - xh * c2);
        }
        *(f32x4*)(dz + (long)dr * ldz + col) = out;
        u += 4;
        while (u >= tp) { u -= tp; ++seg; }
    }
}

// The same pass for a layer without zero frames around its chunks (pad == 0: the dense layers, among them the last frame layer whose
// upstream gradient is the pooling backward - 286 MB at S1, on the critical chain between the loss and the first data-gradient GEMM).
// The loop above loads, computes and stores one row per trip behind two branches, so every trip waits for its own load; here a thread's
// BAF_ROWS / 4 rows are loaded together (addresses clamped instead of predicated) and, POOLED, the statistics of the at most two chunks
// a strip touches are loaded up front and selected per row.  [measured, round 3, r03_elementwise.json] generic form, 1 500 channels:
// 0.62 of 8 TB/s alone, 0.49 in the step (72.6 us for 285.7 MB).
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_apply_dense_kernel(const float* __restrict__ da, PoolGrad pg, const float* __restrict__ z, int rows,
                                                                 int n, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ coef, int relu,
                                                                 float* __restrict__ dz, const float* __restrict__ slope, int ldz /* rows of z and dz */) {
    XV_EW_PRIORITY();
    constexpr int NR = BAF_ROWS / 4;
    const int col = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int rl = threadIdx.x >> 6;
    if (col >= n) return;
    const int r0 = blockIdx.y * BAF_ROWS + rl;
    f32x4 zz[NR], dd[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) zz[j] = *(const f32x4*)(z + (long)min(r0 + 4 * j, rows - 1) * ldz + col);
    if (!POOLED) {
#pragma unroll
        for (int j = 0; j < NR; ++j) dd[j] = *(const f32x4*)(da + (long)min(r0 + 4 * j, rows - 1) * n + col);
    }
    const f32x4 mu = *(const f32x4*)(mean + col), is = *(const f32x4*)(invstd + col);
    const f32x4 sc = *(const f32x4*)(scale + col), sh = *(const f32x4*)(shift + col);
    const f32x4 c1 = *(const f32x4*)(coef + col), c2 = *(const f32x4*)(coef + n + col);
    const f32x4 g_is = *(const f32x4*)(gamma + col) * is;
    const bool hs = slope != nullptr;
    f32x4 sl = {0, 0, 0, 0};
    if (hs) sl = *(const f32x4*)(slope + col);
    PoolCoef pc0 = {}, pc1 = {};
    int b_end = 0;                                  // first row of the strip's second chunk
    float w[NR];
    if (POOLED) {
        const int nb = rows / pg.t;
        const int b0 = min(blockIdx.y * BAF_ROWS / pg.t, nb - 1);
        b_end = (b0 + 1) * pg.t;
        pc0 = pool_coef(pg, b0, n, col);
        pc1 = pool_coef(pg, min(b0 + 1, nb - 1), n, col);
#pragma unroll
        for (int j = 0; j < NR; ++j) w[j] = pg.w ? pg.w[min(r0 + 4 * j, rows - 1)] : 1.f / (float)pg.t;
        // (a strip of BAF_ROWS rows crosses at most one chunk boundary when pg.t >= BAF_ROWS; shorter chunks take the generic kernel)
    }
    if (POOLED && !hs) {
        // Plain ReLU (or none): with a = y where the unit is on, the pooling backward and the BatchNorm backward are both affine in z,
        //   dz = on ? w (A z + B) + (C z + D) : C z + D,   A = g q sc, B = g (dm + q (sh - mean_p)), C = -g is c2, D = g (is c2 mu - c1), g = gamma is
        // - four fused multiply-adds, a compare and a select per element instead of the ~16 operations of the general form below: at 1 500
        // channels x 23 808 rows that form kept the vector ALUs busy for about half of the pass's memory time (0.60 of 8 TB/s alone against
        // 0.73 for the forward pass over the same bytes, r04_elementwise.json).  [measured, same box] 66.9 -> 65.8 us in the step: the pass is not
        // ALU-bound after all; kept for the shorter code path.
        const f32x4 gc2 = g_is * is * c2;
        const f32x4 C = -gc2, D = gc2 * mu - g_is * c1;
        const f32x4 A0 = g_is * (pc0.q * sc), B0 = g_is * (pc0.dm + pc0.q * (sh - pc0.mean));
        const f32x4 A1 = g_is * (pc1.q * sc), B1 = g_is * (pc1.dm + pc1.q * (sh - pc1.mean));
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int r = r0 + 4 * j;
            const bool second = r >= b_end;
            const f32x4 A = second ? A1 : A0, B = second ? B1 : B0;
            const f32x4 y = zz[j] * sc + sh;
            const f32x4 off = C * zz[j] + D;
            f32x4 on = w[j] * (A * zz[j] + B) + off;
            if (relu) {
                on.x = y.x > 0.f ? on.x : off.x; on.y = y.y > 0.f ? on.y : off.y;
                on.z = y.z > 0.f ? on.z : off.z; on.w = y.w > 0.f ? on.w : off.w;
            }
            if (r < rows) *(f32x4*)(dz + (long)r * ldz + col) = on;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int r = r0 + 4 * j;
        f32x4 d;
        if (POOLED) {
            const bool second = r >= b_end;
            d = upstream_grad_pooled(second ? pc1 : pc0, w[j], zz[j], sc, sh, relu, sl, hs);
        } else {
            d = upstream_grad(dd[j], zz[j], sc, sh, relu, sl, hs);
        }
        const f32x4 xh = (zz[j] - mu) * is;
        if (r < rows) *(f32x4*)(dz + (long)r * ldz + col) = g_is * (d - c1 - xh * c2);
    }
}

// Same as bn_bwd_apply_kernel but dz is written as two fp16 planes [2][segs*(t+2pad)][ldd] scaled by the power of two
// derived from *amax (xv_gemm16.h); pad rows / columns are zero.
// Thread = one 8-channel chunk (16 B per plane) x a strip of rows: the 7 per-channel parameter vectors are loaded
// once per thread, not once per element (they were 3/4 of the load instructions of the element-per-thread form).
// block = 64 chunks x 4 row lanes, BAS_ROWS padded rows per block.
#define BAS_ROWS 32
template <bool POOLED>
__global__ __launch_bounds__(256) void bn_bwd_apply_split_kernel(const float* __restrict__ da, PoolGrad pg, const float* __restrict__ z,
                                                                 int segs, int t, int n, const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ scale, const float* __restrict__ shift,
                                                                 const float* __restrict__ coef, int relu, int pad,
                                                                 const unsigned* __restrict__ amax, unsigned short* __restrict__ dst,
                                                                 long ldd, long plane_stride, const float* __restrict__ slope) {
    XV_EW_PRIORITY();
    const float s = xv_pow2_scale(*amax);
    const int tp = t + 2 * pad;
    const int col = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
    const int rl = threadIdx.x >> 6;
    if (col >= ldd) return;
    const int total_rows = segs * tp;
    const int r0 = blockIdx.y * BAS_ROWS, r1 = min(total_rows, r0 + BAS_ROWS);
    f32x4 g_is[2], mu[2], is[2], sc[2], sh[2], c1[2], c2[2], sl[2];
    bool cv[2];
    const bool hs = slope != nullptr;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int c = col + 4 * q;
        cv[q] = c < n;
        const int cc = cv[q] ? c : 0;
        sl[q] = hs ? *(const f32x4*)(slope + cc) : f32x4{0, 0, 0, 0};
        mu[q] = *(const f32x4*)(mean + cc); is[q] = *(const f32x4*)(invstd + cc);
        sc[q] = *(const f32x4*)(scale + cc); sh[q] = *(const f32x4*)(shift + cc);
        c1[q] = *(const f32x4*)(coef + cc); c2[q] = *(const f32x4*)(coef + n + cc);
        g_is[q] = *(const f32x4*)(gamma + cc) * is[q];
    }
    int seg = r0 / tp, u = r0 - seg * tp;          // padded row r0 -> (segment, frame + pad)
    u += rl;
    while (u >= tp) { u -= tp; ++seg; }
    PoolCoef pc[2] = {};
    int b_end = 0;                                 // first row beyond the chunk whose statistics are in pc
    float invT = 0.f;
    for (int dr = r0 + rl; dr < r1; dr += 4) {
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int f = u - pad;
        if (f >= 0 && f < t) {
            const long r = (long)seg * t + f;
            if (POOLED) {
                if (r >= b_end) {
                    const int pb = (int)r / pg.t;
                    b_end = (pb + 1) * pg.t;
#pragma unroll
                    for (int q = 0; q < 2; ++q) pc[q] = pool_coef(pg, pb, n, cv[q] ? col + 4 * q : 0);
                }
                invT = pool_frame_weight(pg, r);
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (!cv[q]) continue;
                const int c = col + 4 * q;
                f32x4 zz = *(const f32x4*)(z + r * n + c);
                f32x4 dd = POOLED ? upstream_grad_pooled(pc[q], invT, zz, sc[q], sh[q], relu, sl[q], hs)
                                  : upstream_grad(*(const f32x4*)(da + r * n + c), zz, sc[q], sh[q], relu, sl[q], hs);
                f32x4 xh = (zz - mu[q]) * is[q];
                f32x4 o = g_is[q] * (dd - c1[q] - xh * c2[q]);
                v[4 * q] = o.x; v[4 * q + 1] = o.y; v[4 * q + 2] = o.z; v[4 * q + 3] = o.w;
            }
        }
        unsigned short h[8], l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float xs = v[j] * s;
            _Float16 hh = (_Float16)xs;
            _Float16 ll = (_Float16)(xs - (float)hh);
            h[j] = __builtin_bit_cast(unsigned short, hh);
            l[j] = __builtin_bit_cast(unsigned short, ll);
        }
        *(uint4*)(dst + (long)dr * ldd + col) = *(const uint4*)h;
        *(uint4*)(dst + plane_stride + (long)dr * ldd + col) = *(const uint4*)l;
        u += 4;
        while (u >= tp) { u -= tp; ++seg; }
    }
}

// BatchNorm backward reductions of a layer that feeds statistics pooling, WITHOUT a pass over z (plain ReLU or no activation).
// With a = act(y), y = gamma*xhat + beta, frame weights omega (1/T or the attention weights, sum 1) and the pooled mean / variance
// (mu, var) of chunk b, the upstream gradient on an active frame is  dd = omega*(dm + q*(a - mu)),  q = dstd/std, and xhat = (a - beta)/gamma
// there; off frames contribute nothing.  Summed over the frames of the chunk, with W+ = the weight on active frames (pooling forward):
//   sum dd        = dm*W+ + q*mu*(1 - W+)
//   sum dd*xhat   = (dm*(mu - beta*W+) + q*(var - beta*mu*(1 - W+))) / gamma
// (sum_on omega*a = mu and sum_on omega*a^2 = var + mu^2 because a = 0 off).  One workgroup = 4 channel quads x 64 chunk lanes (the
// kernel is a handful of dependent memory round trips: 16 quads x 16 lanes, 8 chunks per lane, took 20 us), chunks summed in a fixed
// order; also does bn_bwd_finalize_kernel's job.  gamma == 0 (xhat not recoverable from a) yields inf / nan - loudly.
#define PS_QUADS 4
#define PS_LANES 64
__global__ __launch_bounds__(256) void bn_bwd_pooled_stats_kernel(PoolGrad pg, int segs, int n, int rows, const float* __restrict__ gamma,
                                                                  const float* __restrict__ shift, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  float* __restrict__ coef, float* __restrict__ dbias,
                                                                  const float* __restrict__ zmin, const float* __restrict__ zmax,
                                                                  unsigned* __restrict__ dz_amax) {
    XV_EW_PRIORITY();
    __shared__ f32x4 r1[PS_LANES][PS_QUADS], r2[PS_LANES][PS_QUADS], r3[PS_LANES][PS_QUADS];
    const int cq = threadIdx.x & (PS_QUADS - 1), bl = threadIdx.x / PS_QUADS;
    const int col = (blockIdx.x * PS_QUADS + cq) * 4;
    const bool cv = col < n;
    f32x4 s1 = {0, 0, 0, 0}, s2 = {0, 0, 0, 0}, s3 = {0, 0, 0, 0};
    const float invT = 1.f / (float)pg.t;
    if (cv) {
        // beta = shift + mean*scale (shift = beta - mean*scale, bn_finalize)
        const f32x4 bt = *(const f32x4*)(shift + col) + *(const f32x4*)(mean + col) * *(const f32x4*)(scale + col);
        for (int b = bl; b < segs; b += PS_LANES) {
            const PoolCoef pc = pool_coef(pg, b, n, col);
            const f32x4 sd = *(const f32x4*)(pg.out + (long)b * 2 * n + n + col);
            const f32x4 wp = *(const f32x4*)(pg.wpos + (long)b * n + col);
            const f32x4 off = f32x4{1.f, 1.f, 1.f, 1.f} - wp;
            s1 += pc.dm * wp + pc.q * pc.mean * off;
            s2 += pc.dm * (pc.mean - bt * wp) + pc.q * (sd * sd - bt * pc.mean * off);
            if (dz_amax) {
                // |d a| over the chunk (unit frame weights): d a = (dm + q*(a - mu)) / T is linear in a, a in [0, amax] -> the ends
                const f32x4 am = *(const f32x4*)(pg.amax + (long)b * n + col);
                const f32x4 e0 = pc.dm - pc.q * pc.mean, e1 = pc.dm + pc.q * (am - pc.mean);
                s3 = absmax4(s3, absmax4(__builtin_elementwise_abs(e0), e1) * invT);
            }
        }
    }
    r1[bl][cq] = s1; r2[bl][cq] = s2; r3[bl][cq] = s3;
    __syncthreads();
    if (bl != 0 || !cv) return;
    s1 = r1[0][cq]; s2 = r2[0][cq];
    for (int k = 1; k < PS_LANES; ++k) {
        s1 += r1[k][cq]; s2 += r2[k][cq];
        s3 = absmax4(s3, r3[k][cq]);      // (the lanes' maxima are non-negative)
    }
    const f32x4 g = *(const f32x4*)(gamma + col), is = *(const f32x4*)(invstd + col);
    s2.x /= g.x; s2.y /= g.y; s2.z /= g.z; s2.w /= g.w;
    const float inv_rows = 1.0f / (float)rows;
    const f32x4 c1 = s1 * inv_rows;
    *(f32x4*)(dbeta + col) = s1;
    *(f32x4*)(dgamma + col) = s2;
    *(f32x4*)(coef + col) = c1;
    *(f32x4*)(coef + n + col) = s2 * inv_rows;
    if (dbias) *(f32x4*)(dbias + col) = g * is * (s1 - c1 * (float)rows);
    if (dz_amax) {
        // upper bound of |dz| = |gamma*invstd| * |d a - c1 - xhat*c2| over the batch (bn_bwd_finalize_kernel's, with the analytic |d a| bound)
        const f32x4 mu = *(const f32x4*)(mean + col), zn = *(const f32x4*)(zmin + col), zx = *(const f32x4*)(zmax + col);
        const f32x4 c2 = s2 * inv_rows;
        float bound = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) bound = fmaxf(bound, bn_dz_bound(g[j], is[j], mu[j], zn[j], zx[j], s3[j], c1[j], c2[j]));
        atomicMax(dz_amax, __float_as_uint(bound));
    }
}

// The kernels' view of an upstream-gradient descriptor (xv_bn.h)
static PoolGrad pool_grad_of(const XvBnUpstream& up) {
    return up.pool_out ? PoolGrad{up.pool_out, up.dpool, up.pool_t, up.weights, up.wpos, up.pamax} : PoolGrad{nullptr, nullptr, 1, nullptr, nullptr, nullptr};
}

// Every choice of kernel of the backward, from what the caller has (host arithmetic only).  rows = segs * t; pooled: the upstream gradient is
// the pooling backward over chunks of pool_t frames; has_slope / has_dalpha: the activation context; split: dz as fp16 planes with a |dz|
// bound (dz_amax); ext_chunks > 0: reduction partials a GEMM epilogue left.
//   reduce: closed form from the pooled statistics (needs wpos and no slope; split precision also needs pamax, unit frame weights and no
//           external partials) | external partials | the pooled pass (flags: its RELU, HS, ATT instantiation) | the plain pass
//   nstat:  4 with a slope and a d alpha buffer (prelu), else 3
//   chunks: partial rows the finalize kernel sums (and the workspace holds, unless external)
//   apply:  split planes | dense (pad == 0 and, pooled, chunks of at least one BAF_ROWS strip) | strip
static BnBwdPlan bn_bwd_plan(int rows, bool pooled, int pool_t, int pad, bool relu, bool has_slope, bool has_dalpha, bool has_wpos,
                             bool has_weights, bool split, bool has_pamax, int ext_chunks) {
    BnBwdPlan p;
    const bool slope = relu && has_slope, ext = ext_chunks > 0;
    p.nstat = (slope && has_dalpha) ? 4 : 3;      // prelu: one more reduction, sum d act * min(y, 0)
    // the partials either come from the data-gradient GEMM's epilogue (one chunk per 128-row tile) or are computed into the workspace
    p.chunks = ext ? ext_chunks : pooled ? bn_bwd_pooled_chunks(rows, pool_t) : xv_cdiv(rows, BB_ROWS);
    // statistics pooling behind a plain ReLU (or no activation): reductions and finalize in closed form from the pooled statistics, no pass over z
    bool closed = pooled && has_wpos && !slope;
    // ... whose |dz| bound, where one is wanted, comes from each chunk's largest activation: that needs pamax and unit frame weights, and
    // partials a GEMM epilogue already produced are consumed instead
    if (split) closed = closed && has_pamax && !has_weights && !ext;
    p.reduce = closed ? XV_BNB_CLOSED : ext ? XV_BNB_EXTERNAL : pooled ? XV_BNB_POOLED : XV_BNB_PLAIN;
    p.flags = p.reduce == XV_BNB_POOLED ? (relu ? XV_BNB_RELU : 0) | (slope ? XV_BNB_HS : 0) | (has_weights ? XV_BNB_ATT : 0) : 0;
    p.apply = split ? XV_BNB_SPLIT : (pad == 0 && (!pooled || pool_t >= BAF_ROWS)) ? XV_BNB_DENSE : XV_BNB_STRIP;
    return p;
}
static BnBwdPlan bn_bwd_plan_of(const XvBnUpstream& up, const PoolGrad& pg, int rows, int pad, int relu, const XvActContext& act, bool split) {
    return bn_bwd_plan(rows, pg.out != nullptr, pg.t, pad, relu != 0, act.slope != nullptr, act.dalpha != nullptr, pg.wpos != nullptr,
                       pg.w != nullptr, split, pg.amax != nullptr, up.ext_part ? up.ext_chunks : 0);
}
extern "C" int xv_debug_bn_bwd_plan(int rows, int pooled, int pool_t, int pad, int relu, int has_slope, int has_dalpha, int has_wpos,
                                    int has_weights, int split, int has_pamax, int ext_chunks, int out[5]) {
    XV_REQUIRE(out && rows > 0 && pad >= 0 && ext_chunks >= 0, "debug_bn_bwd_plan: bad arguments");
    XV_REQUIRE(!pooled || (pool_t > 0 && rows % pool_t == 0), "debug_bn_bwd_plan: %d rows are not whole chunks of %d pooled frames", rows, pool_t);
    XV_REQUIRE(!(ext_chunks && relu && has_slope), "debug_bn_bwd_plan: GEMM-epilogue partials only exist for a plain ReLU");
    XV_REQUIRE(!has_dalpha || has_slope, "debug_bn_bwd_plan: a d alpha buffer needs a slope vector");
    const BnBwdPlan p = bn_bwd_plan(rows, pooled != 0, pool_t, pad, relu != 0, has_slope != 0, has_dalpha != 0, has_wpos != 0, has_weights != 0,
                                    split != 0, has_pamax != 0, ext_chunks);
    out[0] = p.reduce; out[1] = p.flags; out[2] = p.nstat; out[3] = p.chunks; out[4] = p.apply;
    return 0;
}

// The reduction stage of both backward forms (each has checked its shape and made the plan): validates the workspace, carves part [chunks][nstat][n] | coef [2][n] out of it,
// reduces the upstream gradient against z - in closed form from the pooled statistics, by the pooled or the plain pass over z, or not at all
// when a GEMM epilogue already left the partials (up.ext_part) - and finalizes: dgamma, dbeta, dbias, d alpha, *coef_out = coef (c1, c2 of
// the apply pass).  dz_amax (split precision, with zmin / zmax): also atomicMax'es the |dz| bound into it, zeroed first if zero_amax.
// `who` names the caller in errors.
static int bn_bwd_reductions(hipStream_t s, const char* who, const BnBwdPlan& plan, const XvBnUpstream& up, const PoolGrad& pg, const float* z,
                             int rows, int n, const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                             const float* zmin, const float* zmax, uint32_t* dz_amax, bool zero_amax, int relu, const XvActContext& act,
                             float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes, const float** coef_out) {
    const float* slope = relu ? act.slope : nullptr;
    const int nstat = plan.nstat, chunks = plan.chunks;
    const size_t part_floats = up.ext_part ? 0 : (size_t)chunks * nstat * n;
    const size_t need = (part_floats + 2 * n) * sizeof(float);
    XV_REQUIRE(need <= ws_bytes, "%s: workspace too small (%zu > %zu)", who, need, ws_bytes);
    float* part = up.ext_part ? const_cast<float*>(up.ext_part) : (float*)ws;
    float* coef = (float*)ws + part_floats;
    *coef_out = coef;
    if (dz_amax && zero_amax) XV_CHECK_HIP(hipMemsetAsync(dz_amax, 0, sizeof(uint32_t), s));
    if (plan.reduce == XV_BNB_CLOSED) {
        hipLaunchKernelGGL(bn_bwd_pooled_stats_kernel, dim3(xv_cdiv(n / 4, PS_QUADS)), dim3(256), 0, s, pg, rows / pg.t, n, rows, gamma, shift, mean,
                           invstd, scale, dgamma, dbeta, coef, dbias, zmin, zmax, (unsigned*)dz_amax);
        XV_LAUNCH_CHECK();
        return 0;
    }
    if (plan.reduce == XV_BNB_POOLED)
        launch_bn_bwd_reduce_pooled(s, pg, z, rows, n, mean, invstd, scale, shift, plan.flags, part, slope, nstat);
    else if (plan.reduce == XV_BNB_PLAIN)
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(xv_cdiv(n / 4, 64), chunks), dim3(256), 0, s,
                           up.da, z, rows, n, mean, invstd, scale, shift, relu, part, slope, nstat);
    if (plan.reduce != XV_BNB_EXTERNAL) XV_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(xv_cdiv(n, FIN_CH)), dim3(256), 0, s, (const float*)part, chunks, n, rows,
                       dgamma, dbeta, coef, gamma, invstd, dbias, mean, zmin, zmax, (unsigned*)dz_amax, nstat,
                       nstat == 4 ? act.dalpha : (float*)nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}

// dz in fp32, segment-padded layout (xv_bn.h).  ldz: leading dimension of z and dz when their rows are padded (the pooled layer: rows on
// the 128-byte grid), 0 = n; closed-form pooled path only.
int xv_bn_backward_f32(hipStream_t s, const XvBnUpstream& up, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                       const float* invstd, const float* scale, const float* shift, int relu, int pad, float* dz_pad, int ldz, float* dgamma,
                       float* dbeta, float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && t > 0 && n > 0 && n % 4 == 0 && pad >= 0, "bn_relu_backward: bad shape (n=%d must be a multiple of 4)", n);
    const PoolGrad pg = pool_grad_of(up);
    const bool pooled = pg.out != nullptr;
    const XvActContext act = xv_act_context();
    const float* slope = relu ? act.slope : nullptr;
    if (ldz == 0) ldz = n;
    XV_REQUIRE(ldz >= n && ldz % 4 == 0 && (ldz == n || (pooled && pg.wpos && !slope)), "bn_relu_backward: a row pitch is only supported on the closed-form pooled path");
    XV_REQUIRE((long)segs * (t + 2 * pad) * (n / 4) < (1L << 31), "bn_relu_backward: tensor too large for 32-bit indexing");
    XV_REQUIRE(!pooled || (pg.t > 0 && (segs * t) % pg.t == 0), "bn_relu_backward: %d rows are not whole chunks of %d pooled frames", segs * t, pg.t);
    XV_REQUIRE(!(up.ext_part && slope), "bn_relu_backward: GEMM-epilogue partials only exist for a plain ReLU");
    const BnBwdPlan plan = bn_bwd_plan_of(up, pg, segs * t, pad, relu, act, false);
    const float* coef = nullptr;
    const int rc = bn_bwd_reductions(s, "bn_relu_backward", plan, up, pg, z, segs * t, n, gamma, mean, invstd, scale, shift, nullptr, nullptr, nullptr,
                                     false, relu, act, dgamma, dbeta, dbias, ws, ws_bytes, &coef);
    if (rc) return rc;
    dim3 agrid(xv_cdiv(n / 4, 64), xv_cdiv(segs * (t + 2 * pad), BAF_ROWS));
    // [measured, round 6, profiles/r06_pooled_kernels.txt] two other forms of the pooled pass were built and dropped: a workgroup per (chunk, 256
    // channels) with the parameters set up once and two batches of eight loads in flight (78 us for statistics + apply alone, as this strip form),
    // and whole-row workgroups that stream consecutive bytes as torch's flat element-wise kernel does (82 us)
    if (plan.apply == XV_BNB_DENSE)
        hipLaunchKernelGGL(pooled ? bn_bwd_apply_dense_kernel<true> : bn_bwd_apply_dense_kernel<false>, agrid, dim3(256), 0, s, up.da, pg, z, segs * t, n,
                           gamma, mean, invstd, scale, shift, coef, relu, dz_pad, slope, ldz);
    else
        hipLaunchKernelGGL(pooled ? bn_bwd_apply_kernel<true> : bn_bwd_apply_kernel<false>, agrid, dim3(256), 0, s, up.da,
                           pg, z, segs, t, n, gamma, mean, invstd, scale, shift, coef, relu, pad, dz_pad, slope, ldz);
    XV_LAUNCH_CHECK();
    return 0;
}

// dz as two fp16 planes scaled by the power of two of *dz_amax, which the reduction stage bounds (xv_bn.h).  zero_amax = false:
// *dz_amax was zeroed by the caller.
int xv_bn_backward_split(hipStream_t s, const XvBnUpstream& up, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                         const float* invstd, const float* scale, const float* shift, const float* zmin, const float* zmax, int relu, int pad,
                         void* dz_planes, int ldp, size_t plane_stride, uint32_t* dz_amax, bool zero_amax, float* dgamma, float* dbeta,
                         float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(segs > 0 && t > 0 && n > 0 && n % 4 == 0 && pad >= 0, "bn_relu_backward_split: bad shape (n=%d must be a multiple of 4)", n);
    XV_REQUIRE(ldp % 8 == 0 && ldp >= n && plane_stride % 8 == 0 && zmin && zmax && dz_amax, "bn_relu_backward_split: bad plane arguments");
    XV_REQUIRE((long)segs * (t + 2 * pad) * (ldp / 8) < (1L << 31), "bn_relu_backward_split: tensor too large for 32-bit indexing");
    const PoolGrad pg = pool_grad_of(up);
    const XvActContext act = xv_act_context();
    XV_REQUIRE(!pg.out || (pg.t > 0 && (segs * t) % pg.t == 0), "bn_relu_backward_split: %d rows are not whole chunks of %d pooled frames", segs * t, pg.t);
    XV_REQUIRE(!(up.ext_part && relu && act.slope), "bn_relu_backward_split: GEMM-epilogue partials only exist for a plain ReLU");
    const BnBwdPlan plan = bn_bwd_plan_of(up, pg, segs * t, pad, relu, act, true);
    const float* coef = nullptr;
    const int rc = bn_bwd_reductions(s, "bn_relu_backward_split", plan, up, pg, z, segs * t, n, gamma, mean, invstd, scale, shift, zmin, zmax, dz_amax,
                                     zero_amax, relu, act, dgamma, dbeta, dbias, ws, ws_bytes, &coef);
    if (rc) return rc;
    dim3 agrid(xv_cdiv(ldp / 8, 64), xv_cdiv(segs * (t + 2 * pad), BAS_ROWS));
    hipLaunchKernelGGL(pg.out ? bn_bwd_apply_split_kernel<true> : bn_bwd_apply_split_kernel<false>, agrid,
                       dim3(256), 0, s, up.da, pg, z, segs, t, n, gamma, mean, invstd, scale, shift, coef, relu, pad,
                       (const unsigned*)dz_amax, (unsigned short*)dz_planes, (long)ldp, (long)plane_stride, relu ? act.slope : nullptr);
    XV_LAUNCH_CHECK();
    return 0;
}

// ---- the op-level C-ABI: each entry point describes its upstream gradient (XvBnUpstream: da | pool_out, dpool, pool_t, weights, wpos,
// pamax | ext_part, ext_chunks) and calls one of the two forms ----
extern "C" int xv_bn_relu_backward(void* stream, const float* da, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                                   const float* invstd, const float* scale, const float* shift, int relu, int pad, float* dz_pad, float* dgamma,
                                   float* dbeta, float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(da, "bn_relu_backward: null upstream gradient");
    return xv_bn_backward_f32((hipStream_t)stream, XvBnUpstream{da}, z, segs, t, n, gamma, mean, invstd, scale, shift, relu, pad, dz_pad, 0, dgamma,
                              dbeta, dbias, ws, ws_bytes);
}

extern "C" int xv_bn_relu_backward_split(void* stream, const float* da, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                                         const float* invstd, const float* scale, const float* shift, const float* zmin, const float* zmax, int relu,
                                         int pad, void* dz_planes, int ldp, size_t plane_stride, uint32_t* dz_amax, float* dgamma, float* dbeta,
                                         float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(da, "bn_relu_backward_split: null upstream gradient");
    return xv_bn_backward_split((hipStream_t)stream, XvBnUpstream{da}, z, segs, t, n, gamma, mean, invstd, scale, shift, zmin, zmax, relu, pad,
                                dz_planes, ldp, plane_stride, dz_amax, true, dgamma, dbeta, dbias, ws, ws_bytes);
}

// xv_bn_relu_backward_split with the reduction partials already produced by xv_affine_dgrad_bnstats_f16x3 (the pass over
// (da, z) that computes them is skipped): part [chunks][3][n], chunks = ceil(rows / 128), ReLU layers, pad as usual.
extern "C" int xv_bn_relu_backward_split_from_part(void* stream, const float* part, int chunks, const float* da, const float* z, int segs, int t, int n,
                                                   const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                                                   const float* zmin, const float* zmax, int pad, void* dz_planes, int ldp, size_t plane_stride,
                                                   uint32_t* dz_amax, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(da && part && chunks == xv_cdiv(segs * t, XV_TILE_M), "bn_relu_backward_split_from_part: one chunk per 128-row tile expected");
    const XvBnUpstream up = {da, nullptr, nullptr, 0, nullptr, nullptr, nullptr, part, chunks};
    return xv_bn_backward_split((hipStream_t)stream, up, z, segs, t, n, gamma, mean, invstd, scale, shift, zmin, zmax, 1, pad, dz_planes, ldp,
                                plane_stride, dz_amax, true, dgamma, dbeta, dbias, ws, ws_bytes);
}

extern "C" int xv_bn_relu_backward_pooled(void* stream, const float* pool_out, const float* dpool, const float* weights, int b, int t, const float* z,
                                          int n, const float* gamma, const float* mean, const float* invstd, const float* scale, const float* shift,
                                          int relu, float* dz, float* dgamma, float* dbeta, float* dbias, void* ws, size_t ws_bytes) {
    XV_REQUIRE(pool_out && dpool && b > 0 && t > 0, "bn_relu_backward_pooled: bad arguments");
    return xv_bn_backward_f32((hipStream_t)stream, XvBnUpstream{nullptr, pool_out, dpool, t, weights}, z, b * t, 1, n, gamma, mean, invstd, scale, shift,
                              relu, 0, dz, 0, dgamma, dbeta, dbias, ws, ws_bytes);
}
// wpos from xv_stat_pool_forward_bn_aux: the reductions then need no pass over z
extern "C" int xv_bn_relu_backward_pooled_aux(void* stream, const float* pool_out, const float* dpool, const float* weights, const float* wpos, int b,
                                              int t, const float* z, int n, const float* gamma, const float* mean, const float* invstd,
                                              const float* scale, const float* shift, int relu, float* dz, float* dgamma, float* dbeta, float* dbias,
                                              void* ws, size_t ws_bytes) {
    XV_REQUIRE(wpos, "bn_relu_backward_pooled_aux: wpos is required");
    XV_REQUIRE(pool_out && dpool && b > 0 && t > 0, "bn_relu_backward_pooled: bad arguments");
    return xv_bn_backward_f32((hipStream_t)stream, XvBnUpstream{nullptr, pool_out, dpool, t, weights, wpos}, z, b * t, 1, n, gamma, mean, invstd, scale,
                              shift, relu, 0, dz, 0, dgamma, dbeta, dbias, ws, ws_bytes);
}

extern "C" int xv_bn_relu_backward_pooled_split(void* stream, const float* pool_out, const float* dpool, const float* weights, int b, int t,
                                                const float* z, int n, const float* gamma, const float* mean, const float* invstd, const float* scale,
                                                const float* shift, const float* zmin, const float* zmax, int relu, void* dz_planes, int ldp,
                                                size_t plane_stride, uint32_t* dz_amax, float* dgamma, float* dbeta, float* dbias, void* ws,
                                                size_t ws_bytes) {
    XV_REQUIRE(pool_out && dpool && b > 0 && t > 0, "bn_relu_backward_pooled_split: bad arguments");
    return xv_bn_backward_split((hipStream_t)stream, XvBnUpstream{nullptr, pool_out, dpool, t, weights}, z, b * t, 1, n, gamma, mean, invstd, scale,
                                shift, zmin, zmax, relu, 0, dz_planes, ldp, plane_stride, dz_amax, true, dgamma, dbeta, dbias, ws, ws_bytes);
}
