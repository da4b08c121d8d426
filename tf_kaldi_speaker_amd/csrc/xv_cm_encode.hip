// Kaldi 'CM ' compressed-matrix ENCODE on the GPU: the other half of the codec of xv_prep.hip (cm_decode_kernel), what
// copy-feats --compress=true does behind the feature pipe of the reference recipe (egs/voxceleb/v1/run.sh stage 4,
// prepare_feats_for_egs.sh) and what dataset/kaldi_io.py write_compressed_mat does on the host - that function is the specification,
// byte for byte, in both header forms (include/xvector_hip.h states the rules).  Every operation is the host writer's, one at a time in
// the order written, with no contraction (fp contract off) and the correctly rounded fp32 division hipcc emits by default.
//
// One workgroup per piece, 32 columns x 8 rows of threads, the columns walked in groups of 32 (d = 128: four groups); a row of a group
// is read as one run of up to 128 bytes.  The piece is streamed a fixed number of times from L2 / HBM and none of it is kept in LDS, so
// rows is not bounded by LDS:
//   1. column minima and maxima (exact in any order), from them the matrix minimum and range;
//   2. quartiles, rows >= 5: the order statistics at ranks rows / 4 and 3 rows / 4 of every column, EXACTLY, by radix select over the
//      order-preserving key (xv_radix_key.h), most significant byte first: four passes per rank, a 256-bin histogram per column in LDS
//      (bin-major, so the 32 columns of a wave's row fall into 32 banks whatever the digit), INTEGER atomics only - a count does not
//      depend on the order of its increments.  rows < 5: a thread per column sorts its four values.  uniform: nothing, step 1 has it;
//   3. a thread per column maps its points to uint16, applies the strictly-increasing fix-up and writes the column header bytewise
//      (an image may start at any byte);
//   4. the codes: tiles of 64 rows are coded along d (how x is stored), transposed through LDS and stored along the rows (how the
//      image is stored), a wave writing 64 consecutive bytes.
// No floating-point atomics and no cross-workgroup hand-over: the bytes depend on the shape of the call only.  gfx950 only.
#include <cmath>

#include "xv_common.h"
#include "xv_radix_key.h"

#define CME_MAX_D 128
#define CME_CG 32          // columns per group = threads along d
#define CME_RY 8           // threads along the rows
#define CME_RT 64          // rows per tile of the code pass

__device__ __forceinline__ void cme_put16(uint8_t* p, unsigned u) { p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); }
__device__ __forceinline__ void cme_put32(uint8_t* p, unsigned u) { cme_put16(p, u); cme_put16(p + 2, u >> 16); }
__device__ __forceinline__ void cme_swap(float& a, float& b) { const float lo = fminf(a, b), hi = fmaxf(a, b); a = lo; b = hi; }

// v[u] = column c of row r0 + CME_RY u for u < CME_U, the loads issued together (a workgroup streams its piece alone: what hides the
// latency of a load is the loads behind it); a row at or behind n gives row r0 again (r0 < n), so nothing outside the piece is read.
#define CME_U 8
static_assert(CME_RT == CME_RY * CME_U, "a thread codes the CME_U rows of a tile it loaded together");
__device__ __forceinline__ void cme_load(const float* __restrict__ xp, int D, int c, int r0, int n, float v[CME_U]) {
#pragma unroll
    for (int u = 0; u < CME_U; ++u) {
        const int r = r0 + CME_RY * u;
        v[u] = xp[(long)(r < n ? r : r0) * D + c];
    }
}

__global__ __launch_bounds__(256) void cm_encode_kernel(const float* __restrict__ x, const int* __restrict__ rows, const long* __restrict__ offs,
                                                        uint8_t* __restrict__ out, int T, int D, int uniform) {
#pragma clang fp contract(off)
    __shared__ unsigned hist[256 * CME_CG];              // [bin][column of the group]
    __shared__ unsigned seg[CME_RY * CME_CG];            // the counts of 32 bins each
    __shared__ unsigned sel_prefix[CME_CG], sel_rank[CME_CG];
    __shared__ float red[2][CME_RY][CME_CG];
    __shared__ float cmin[CME_MAX_D], cmax[CME_MAX_D];
    __shared__ float q[3][CME_MAX_D];                    // the inner order statistics (rows < 5: the 2nd, 3rd and 4th smallest value)
    __shared__ float pt[4][CME_MAX_D];                   // the four float points of a column
    __shared__ uint8_t tile[CME_CG][CME_RT + 4];
    const int tid = threadIdx.x, tx = tid & (CME_CG - 1), ty = tid / CME_CG;
    const int n = rows[blockIdx.x];
    const float* xp = x + (long)blockIdx.x * T * D;
    uint8_t* o = out + offs[blockIdx.x];
    const int groups = (D + CME_CG - 1) / CME_CG;

    // 1. column minima and maxima over the n valid rows
    for (int g = 0; g < groups; ++g) {
        const int c = g * CME_CG + tx;
        float lo = INFINITY, hi = -INFINITY;
        if (c < D)
            for (int r0 = ty; r0 < n; r0 += CME_RY * CME_U) {
                float v[CME_U];
                cme_load(xp, D, c, r0, n, v);
#pragma unroll
                for (int u = 0; u < CME_U; ++u) {      // a repeated row changes neither
                    lo = fminf(lo, v[u]);
                    hi = fmaxf(hi, v[u]);
                }
            }
        red[0][ty][tx] = lo;
        red[1][ty][tx] = hi;
        __syncthreads();
        if (ty == 0 && c < D) {
            for (int k = 1; k < CME_RY; ++k) {
                lo = fminf(lo, red[0][k][tx]);
                hi = fmaxf(hi, red[1][k][tx]);
            }
            cmin[c] = lo;
            cmax[c] = hi;
        }
        __syncthreads();
    }
    float gmin = INFINITY, gmax = -INFINITY;
    for (int c = 0; c < D; ++c) {
        gmin = fminf(gmin, cmin[c]);
        gmax = fmaxf(gmax, cmax[c]);
    }
    const float grange = gmax == gmin ? (float)((double)gmin + 1.0 + fabs((double)gmin) - (double)gmin) : (float)((double)gmax - (double)gmin);

    // 2. the inner order statistics of the quartile header
    if (!uniform && n < 5) {
        for (int c = tid; c < D; c += 256) {
            float v[4];
            for (int k = 0; k < 4; ++k) v[k] = k < n ? xp[(long)k * D + c] : INFINITY;
            cme_swap(v[0], v[1]); cme_swap(v[2], v[3]); cme_swap(v[0], v[2]); cme_swap(v[1], v[3]); cme_swap(v[1], v[2]);
            q[0][c] = v[1]; q[1][c] = v[2]; q[2][c] = v[3];
        }
    } else if (!uniform) {
        for (int g = 0; g < groups; ++g) {
            const int c = g * CME_CG + tx;
            for (int j = 0; j < 2; ++j) {
                if (tid < CME_CG) {
                    sel_prefix[tid] = 0u;
                    sel_rank[tid] = (unsigned)(j == 0 ? n / 4 : (int)(3 * (long)n / 4));
                }
                for (int pass = 0; pass < 4; ++pass) {
                    const int shift = 24 - 8 * pass;
                    for (int i = tid; i < 256 * CME_CG; i += 256) hist[i] = 0u;
                    __syncthreads();
                    if (c < D) {
                        const unsigned prefix = sel_prefix[tx];
                        for (int r0 = ty; r0 < n; r0 += CME_RY * CME_U) {
                            float v[CME_U];
                            cme_load(xp, D, c, r0, n, v);
#pragma unroll
                            for (int u = 0; u < CME_U; ++u) {
                                const unsigned key = sc_key(v[u]);
                                if (r0 + CME_RY * u < n && (pass == 0 || (key >> (shift + 8)) == prefix))
                                    atomicAdd(&hist[((key >> shift) & 255u) * CME_CG + tx], 1u);
                            }
                        }
                    }
                    __syncthreads();
                    {
                        unsigned s = 0u;
                        for (int k = 0; k < 32; ++k) s += hist[(ty * 32 + k) * CME_CG + tx];
                        seg[ty * CME_CG + tx] = s;
                    }
                    __syncthreads();
                    if (tid < CME_CG) {      // the bin that holds the rank: first the run of 32 bins, then the bin (both walks are bounded)
                        const unsigned k = sel_rank[tid];
                        unsigned cum = 0u;
                        int s = 0;
                        while (s < CME_RY - 1 && cum + seg[s * CME_CG + tid] <= k) cum += seg[s++ * CME_CG + tid];
                        int bin = s * 32;
                        const int last = bin + 31;
                        while (bin < last && cum + hist[bin * CME_CG + tid] <= k) cum += hist[bin++ * CME_CG + tid];
                        sel_prefix[tid] = (sel_prefix[tid] << 8) | (unsigned)bin;
                        sel_rank[tid] = k - cum;
                    }
                    __syncthreads();
                }
                if (ty == 0 && c < D) q[j][c] = sc_unkey(sel_prefix[tx]);
                __syncthreads();
            }
        }
    }
    __syncthreads();

    // 3. headers
    if (tid == 0) {
        cme_put32(o, __float_as_uint(gmin));
        cme_put32(o + 4, __float_as_uint(grange));
        cme_put32(o + 8, (unsigned)n);
        cme_put32(o + 12, (unsigned)D);
    }
    for (int c = tid; c < D; c += 256) {
        int p[4];
        if (uniform) {
            const double f0 = ((double)cmin[c] - (double)gmin) / (double)grange * 65535.0;
            const double f100 = ((double)cmax[c] - (double)gmin) / (double)grange * 65535.0;
            const double p0 = fmin(fmax(floor(f0), 0.0), 65535.0), p100 = fmin(fmax(ceil(f100), 0.0), 65535.0);
            p[0] = (int)p0;
            p[1] = (int)rint(p0 + 0.25 * (p100 - p0));
            p[2] = (int)rint(p0 + 0.75 * (p100 - p0));
            p[3] = (int)p100;
        } else {
            auto u16 = [&](float v) {
                const float f = (v - gmin) / grange;
                const float s = f * 65535.0f + 0.499f;
                return (int)fminf(fmaxf(floorf(s), 0.0f), 65535.0f);
            };
            p[0] = u16(cmin[c]);
            if (n >= 5) {
                p[1] = u16(q[0][c]); p[2] = u16(q[1][c]); p[3] = u16(cmax[c]);
            } else {      // the small-matrix branch: the order statistics there are, then + 1 in uint16 arithmetic (it wraps)
                p[1] = n > 1 ? u16(q[0][c]) : ((p[0] + 1) & 0xffff);
                p[2] = n > 2 ? u16(q[1][c]) : ((p[1] + 1) & 0xffff);
                p[3] = n > 3 ? u16(q[2][c]) : ((p[2] + 1) & 0xffff);
            }
        }
        p[0] = min(p[0], 65532);
        p[1] = min(max(p[1], p[0] + 1), 65533);
        p[2] = min(max(p[2], p[1] + 1), 65534);
        p[3] = max(p[3], p[2] + 1);
        const float gs = grange * 1.52590218966964e-05f;        // 1/65535
        for (int k = 0; k < 4; ++k) {
            cme_put16(o + 16 + 8 * c + 2 * k, (unsigned)p[k]);
            pt[k][c] = gmin + gs * (float)p[k];
        }
    }
    __syncthreads();

    // 4. the codes, column after column
    uint8_t* data = o + 16 + 8 * (long)D;
    for (int g = 0; g < groups; ++g) {
        const int c = g * CME_CG + tx;
        float f0 = 0.f, f25 = 0.f, f75 = 0.f, f100 = 0.f;
        if (c < D) { f0 = pt[0][c]; f25 = pt[1][c]; f75 = pt[2][c]; f100 = pt[3][c]; }
        for (int r0 = 0; r0 < n; r0 += CME_RT) {
            const int rt = min(CME_RT, n - r0);
            __syncthreads();
            if (c < D && ty < rt) {
                float vs[CME_U];
                cme_load(xp, D, c, r0 + ty, n, vs);
#pragma unroll
                for (int u = 0; u < CME_U; ++u) {
                    const int rl = ty + CME_RY * u;
                    if (rl >= rt) break;
                    const float v = vs[u];
                    float code;      // fminf / fmaxf drop a NaN (two coinciding points: 0 / 0), so the code stays inside its branch's range
                    if (v < f25) code = fminf(fmaxf(floorf((v - f0) / (f25 - f0) * 64.0f + 0.5f), 0.0f), 64.0f);
                    else if (v < f75) code = fminf(fmaxf(64.0f + floorf((v - f25) / (f75 - f25) * 128.0f + 0.5f), 64.0f), 192.0f);
                    else code = fminf(fmaxf(192.0f + floorf((v - f75) / (f100 - f75) * 63.0f + 0.5f), 192.0f), 255.0f);
                    tile[tx][rl] = (uint8_t)(int)code;
                }
            }
            __syncthreads();
            for (int idx = tid; idx < CME_CG * CME_RT; idx += 256) {
                const int cl = idx / CME_RT, rl = idx - cl * CME_RT, cc = g * CME_CG + cl;
                if (cc < D && rl < rt) data[(long)cc * n + r0 + rl] = tile[cl][rl];
            }
        }
    }
}

extern "C" int xv_cm_encode(void* stream, const float* x, const int32_t* rows, int b, int t, int d, int header, const int64_t* out_offsets,
                            uint8_t* out) {
    XV_REQUIRE(x && rows && out_offsets && out && b > 0 && t > 0 && d > 0, "cm_encode: bad arguments");
    XV_REQUIRE(d <= CME_MAX_D, "cm_encode: at most %d feature dimensions (got %d)", CME_MAX_D, d);
    XV_REQUIRE(header == XV_CM_HEADER_QUARTILES || header == XV_CM_HEADER_UNIFORM, "cm_encode: header must be XV_CM_HEADER_QUARTILES or XV_CM_HEADER_UNIFORM (got %d)", header);
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    hipLaunchKernelGGL(cm_encode_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, x, (const int*)rows, (const long*)out_offsets, out, t, d,
                       header == XV_CM_HEADER_UNIFORM);
    XV_LAUNCH_CHECK();
    return 0;
}
