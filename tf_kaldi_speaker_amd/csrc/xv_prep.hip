// Input and weight preparation: the Kaldi 'CM ' decode of packed feature batches, the kernel-layout copies of the weights (forward
// transpose, tap-flipped data-gradient layout; fp32 or fp16 planes; one launch for all layers of a step) and the multi-tensor max |x|
// that scales the planes.  These kernels fill a side stream with slack (XV_EW_FILLER, xv_common.h).  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_epilogue.h"
#include "xv_prep.h"

// ------------------------------------------------------------------------------------
// Kaldi 'CM ' compressed-matrix decode on the GPU (kaldi_io.py:768-867 / compressed-matrix.h) for batches the native loader delivers
// packed (include/xvector_io.h: per chunk [min f32][range f32][D x (p0, p25, p75, p100) u16][D x T u8, column after column], padded to
// `stride` bytes).  One workgroup per chunk: the column parameters once, then tiles of CMD_TT frames - bytes in along the frame axis
// (how they are stored), floats out along the feature axis (how [b][t][d] is stored), transposed through LDS.
// The arithmetic is the reference codec's, operation by operation in float with no contraction (fp contract off), so the result is
// bit-identical to the host decoder (xv_loader.cpp, -ffp-contract=off) and to the reference reader.
// ------------------------------------------------------------------------------------
#define CMD_MAX_D 128
#define CMD_TT 128
// Ragged form (batched extraction: whole utterances of different lengths): chunk i starts at byte offs[i], holds rows[i] frames (its bytes
// are [D][rows[i]]) and is written to out[i][0 .. rows[i]) of a [b][T][D] tensor whose remaining rows are zeroed.  hdr = bytes in front
// of the column headers: 8 (min, range: the native loader's packing) or 16 (min, range, rows, cols: the matrix as it sits in the archive).
__global__ __launch_bounds__(256) void cm_decode_kernel(const uint8_t* __restrict__ packed, long stride, int T, int D, float* __restrict__ out,
                                                        const long* __restrict__ offs, const int* __restrict__ rows, int hdr) {
#pragma clang fp contract(off)
    XV_EW_FILLER();
    __shared__ float prm[6][CMD_MAX_D];                  // p0, p25, p75, s_lo, s_mid, s_hi per column
    __shared__ uint8_t tile[CMD_MAX_D][CMD_TT + 4];
    const uint8_t* chunk = packed + (offs ? offs[blockIdx.x] : (long)blockIdx.x * stride);
    const int tid = threadIdx.x;
    const int Tout = T;
    if (rows) {
        T = min(T, rows[blockIdx.x]);
        float* pad = out + ((long)blockIdx.x * Tout + T) * D;
        for (long i = tid; i < (long)(Tout - T) * D; i += 256) pad[i] = 0.f;
    }
    float minv, range;
    memcpy(&minv, chunk, 4);
    memcpy(&range, chunk + 4, 4);
    // plain operators under "fp contract(off)": HIP's __fmul_rn / __fadd_rn are inline functions compiled with the default contraction,
    // and their multiply-adds get fused into v_fma_f32 after inlining (1 ulp off the codec)
    const float gs = range * 1.52590218966964e-05f;        // 1/65535
    if (tid < D) {
        unsigned short h[4];
        memcpy(h, chunk + hdr + 8 * tid, 8);
        const float p0 = minv + gs * (float)h[0], p25 = minv + gs * (float)h[1];
        const float p75 = minv + gs * (float)h[2], p100 = minv + gs * (float)h[3];
        prm[0][tid] = p0; prm[1][tid] = p25; prm[2][tid] = p75;
        prm[3][tid] = (p25 - p0) / 64.0f;
        prm[4][tid] = (p75 - p25) / 128.0f;
        prm[5][tid] = (p100 - p75) / 63.0f;
    }
    const uint8_t* bytes = chunk + hdr + 8 * (long)D;
    float* o = out + (long)blockIdx.x * Tout * D;
    for (int t0 = 0; t0 < T; t0 += CMD_TT) {
        const int tt_n = min(CMD_TT, T - t0);
        __syncthreads();
        for (int idx = tid; idx < D * CMD_TT; idx += 256) {
            const int d = idx / CMD_TT, tt = idx - d * CMD_TT;
            if (tt < tt_n) tile[d][tt] = bytes[(long)d * T + t0 + tt];
        }
        __syncthreads();
        for (int idx = tid; idx < tt_n * D; idx += 256) {
            const int tt = idx / D, d = idx - tt * D;
            const uint8_t b = tile[d][tt];
            const float v = (float)b;
            float y;
            if (b <= 64) y = prm[0][d] + prm[3][d] * v;
            else if (b <= 192) y = prm[1][d] + prm[4][d] * (v - 64.0f);
            else y = prm[2][d] + prm[5][d] * (v - 192.0f);
            o[(long)(t0 + tt) * D + d] = y;
        }
    }
}

extern "C" int xv_cm_decode(void* stream, const uint8_t* packed, int b, int t, int d, size_t chunk_stride, float* out) {
    XV_REQUIRE(packed && out && b > 0 && t > 0 && d > 0, "cm_decode: bad arguments");
    XV_REQUIRE(d <= CMD_MAX_D, "cm_decode: at most %d feature dimensions (got %d)", CMD_MAX_D, d);
    XV_REQUIRE(chunk_stride >= (size_t)8 + 8 * (size_t)d + (size_t)d * t, "cm_decode: chunk stride %zu is smaller than a chunk", chunk_stride);
    hipLaunchKernelGGL(cm_decode_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, packed, (long)chunk_stride, t, d, out, (const long*)nullptr,
                       (const int*)nullptr, 8);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_cm_decode_ragged(void* stream, const uint8_t* packed, const int64_t* offsets, const int32_t* rows, int b, int t, int d, float* out) {
    XV_REQUIRE(packed && offsets && rows && out && b > 0 && t > 0 && d > 0, "cm_decode_ragged: bad arguments");
    XV_REQUIRE(d <= CMD_MAX_D, "cm_decode_ragged: at most %d feature dimensions (got %d)", CMD_MAX_D, d);
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    hipLaunchKernelGGL(cm_decode_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, packed, 0L, t, d, out, (const long*)offsets, (const int*)rows, 16);
    XV_LAUNCH_CHECK();
    return 0;
}

// wt[o][j*c_pad + c] = kernel[(j*C + c)*O + o], zero for c >= C.  32x32 LDS-tiled transpose:
// reads run along o (contiguous in kernel), writes run along the padded k axis (contiguous in wt).
__global__ void prep_weight_fwd_kernel(const float* __restrict__ w, int k, int C, int O, float* __restrict__ wt, int c_pad) {
    XV_EW_FILLER();
    __shared__ float tile[32][33];
    const int kp = k * c_pad;
    const int kk0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        int kk = kk0 + r, o = o0 + tx;
        float v = 0.f;
        if (kk < kp && o < O) {
            int j = kk / c_pad, c = kk - j * c_pad;
            if (c < C) v = w[((long)j * C + c) * O + o];
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        int o = o0 + r, kk = kk0 + tx;
        if (o < O && kk < kp) wt[(long)o * kp + kk] = tile[tx][r];
    }
}

extern "C" int xv_prep_weight_fwd(void* stream, const float* kernel, int k, int c, int o, float* wt, int c_pad) {
    XV_REQUIRE(k > 0 && c > 0 && o > 0 && c_pad >= c, "prep_weight_fwd: bad shape");
    dim3 grid(xv_cdiv((long)k * c_pad, 32), xv_cdiv(o, 32));
    hipLaunchKernelGGL(prep_weight_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, kernel, k, c, o, wt, c_pad);
    XV_LAUNCH_CHECK();
    return 0;
}

__global__ void prep_weight_dgrad_kernel(const float* __restrict__ w, int k, int C, int O, float* __restrict__ wf) {
    XV_EW_FILLER();
    long total = (long)k * C * O;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int o = (int)(i % O);
        long jc = i / O;
        int c = (int)(jc % C), j = (int)(jc / C);
        wf[(long)c * k * O + (long)(k - 1 - j) * O + o] = w[i];
    }
}

extern "C" int xv_prep_weight_dgrad(void* stream, const float* kernel, int k, int c, int o, float* wf) {
    XV_REQUIRE(k > 0 && c > 0 && o > 0, "prep_weight_dgrad: bad shape");
    long total = (long)k * c * o;
    hipLaunchKernelGGL(prep_weight_dgrad_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, kernel, k, c, o, wf);
    XV_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------
// multi-job weight preparation (xv_prep.h): one launch for every layout copy of every layer
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void weight_prep_multi_kernel(XvPrepJobs J) {
    XV_EW_FILLER();
    __shared__ float tile[32][33];
    int ji = 0;
#pragma unroll 1
    for (int i = 1; i < J.n; ++i) if ((int)blockIdx.x >= J.j[i].tile0) ji = i;
    const XvPrepJob& q = J.j[ji];
    const int lt = blockIdx.x - q.tile0;
    const int txt = lt % q.tiles_x, tyt = lt / q.tiles_x;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    if (q.type == XV_PREP_PAD) {
        // rows r0 .. r0 + 31 of [O][C] -> [O][c_pad], columns c0 .. c0 + 31 (pad columns zero)
        const int r0 = tyt * 32, c = txt * 32 + tx;
        if (c < q.c_pad)
            for (int r = r0 + ty; r < min(r0 + 32, q.O); r += 8) ((float*)q.dst)[(long)r * q.c_pad + c] = c < q.C ? q.w[(long)r * q.C + c] : 0.f;
        return;
    }
    const bool planes = q.type >= XV_PREP_T16 && q.type != XV_PREP_PAD;
    const float sc = planes ? xv_pow2_scale(*q.amax) : 1.0f;
    if (q.type == XV_PREP_T32 || q.type == XV_PREP_T16) {
        // transpose through LDS: reads run along o (contiguous in w), writes along the padded k axis
        const int kp = q.k * q.c_pad;
        const int kk0 = txt * 32, o0 = tyt * 32;
        for (int r = ty; r < 32; r += 8) {
            int kk = kk0 + r, o = o0 + tx;
            float v = 0.f;
            if (kk < kp && o < q.O) {
                int j = kk / q.c_pad, c = kk - j * q.c_pad;
                if (c < q.C) v = q.w[((long)j * q.C + c) * q.O + o];
            }
            tile[r][tx] = v;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            int o = o0 + r, kk = kk0 + tx;
            if (o < q.O && kk < kp) {
                float v = tile[tx][r];
                if (!planes) ((float*)q.dst)[(long)o * kp + kk] = v;
                else {
                    float xs = v * sc;
                    _Float16 h = (_Float16)xs, l = (_Float16)(xs - (float)h);
                    unsigned short* d = (unsigned short*)q.dst;
                    d[(long)o * kp + kk] = __builtin_bit_cast(unsigned short, h);
                    d[q.plane + (long)o * kp + kk] = __builtin_bit_cast(unsigned short, l);
                }
            }
        }
    } else {
        // tap flip, no transpose: rows jc = j*C + c of w, columns o (pad columns o in [O, o_ld) are zero)
        const int jc0 = tyt * 32, o0 = txt * 32;
        const long ldd = (long)q.k * q.o_ld;
        for (int r = ty; r < 32; r += 8) {
            int jc = jc0 + r, o = o0 + tx;
            if (jc < q.k * q.C && o < q.o_ld) {
                int j = jc / q.C, c = jc - j * q.C;
                float v = o < q.O ? q.w[(long)jc * q.O + o] : 0.f;
                long di = (long)c * ldd + (long)(q.k - 1 - j) * q.o_ld + o;
                if (!planes) ((float*)q.dst)[di] = v;
                else {
                    float xs = v * sc;
                    _Float16 h = (_Float16)xs, l = (_Float16)(xs - (float)h);
                    unsigned short* d = (unsigned short*)q.dst;
                    d[di] = __builtin_bit_cast(unsigned short, h);
                    d[q.plane + di] = __builtin_bit_cast(unsigned short, l);
                }
            }
        }
    }
}

int xv_prep_add(XvPrepJobs& J, int type, const float* w, int k, int C, int O, int c_pad, int o_ld, void* dst, long plane,
                const unsigned* amax) {
    XV_REQUIRE(J.n < XV_PREP_MAX_JOBS, "weight_prep: too many jobs");
    XvPrepJob& q = J.j[J.n++];
    q.type = type; q.k = k; q.C = C; q.O = O; q.c_pad = c_pad; q.o_ld = o_ld; q.w = w; q.dst = dst; q.plane = plane; q.amax = amax;
    int tiles_y;
    if (type == XV_PREP_PAD) { q.tiles_x = xv_cdiv(c_pad, 32); tiles_y = xv_cdiv(O, 32); }
    else if (type == XV_PREP_T32 || type == XV_PREP_T16) { q.tiles_x = xv_cdiv((long)k * c_pad, 32); tiles_y = xv_cdiv(O, 32); }
    else { q.tiles_x = xv_cdiv(o_ld, 32); tiles_y = xv_cdiv((long)k * C, 32); }
    q.tile0 = J.total_tiles;
    J.total_tiles += q.tiles_x * tiles_y;
    return 0;
}

int xv_launch_weight_prep(hipStream_t s, const XvPrepJobs& J) {
    if (J.n == 0) return 0;
    hipLaunchKernelGGL(weight_prep_multi_kernel, dim3(J.total_tiles), dim3(256), 0, s, J);
    XV_LAUNCH_CHECK();
    return 0;
}

// max |x| of up to 8 tensors in one launch: blockIdx.y = tensor, one atomicMax per workgroup (slots zeroed by the caller)
__global__ __launch_bounds__(256) void amax_multi_kernel(XvAmaxJobs J) {
    XV_EW_FILLER();
    __shared__ float red[4];
    const float* x = J.x[blockIdx.y];
    const size_t count = J.count[blockIdx.y];
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        unsigned bits = __float_as_uint(m);
        unsigned* out = J.out[blockIdx.y];
        if (bits > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, bits);
    }
}

int xv_launch_amax_multi(hipStream_t s, const XvAmaxJobs& J) {
    if (J.n == 0) return 0;
    hipLaunchKernelGGL(amax_multi_kernel, dim3(256, J.n), dim3(256), 0, s, J);
    XV_LAUNCH_CHECK();
    return 0;
}
