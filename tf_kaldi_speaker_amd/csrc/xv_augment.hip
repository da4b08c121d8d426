// Reverberation and additive-noise augmentation of waveforms - what wav-reverberate (--normalize-output=true) does for the training list
// of the recipe (egs/voxceleb/v1/run.sh:68-130).  Kaldi is not available where this project is built and tested: parity is BY
// RESTATEMENT.  include/xvector_hip.h states the arithmetic, tests/augment_ref.py restates it in fp64, the kernels are held against that.
//
// Direct-form FIR, not FFT.  Kaldi convolves in FFT blocks; this unit does not: a direct form has a short add chain that can be stated
// (XV_AUG_KB + ceil(L / XV_AUG_KB) roundings) and needs no twiddle tables.  From the flop count (2 n L: ~2 GFLOP for 8 s under 8 000
// taps) an utterance is tens of microseconds, far under the host's wav reading: measured at 0.21 of the fp32 vector rate, 62 us for that
// utterance (profiles/augment_bench.txt); the FFT form (overlap-save on xv_mfcc's wave FFT) was not tried.
//
// aug_fir_kernel: one workgroup per tile of XV_AUG_TILE outputs, a lane owning AUG_R consecutive ones.  The taps go through LDS in chunks
// of AUG_KC beside the AUG_TILE + AUG_KC - 1 source samples they meet, int16 -> fp32 once when staged, zeros outside [0, n) written by
// the staging.  Per block of XV_AUG_KB taps a lane reads its window of AUG_R + XV_AUG_KB - 1 samples into registers (every index static),
// the taps arrive as LDS broadcasts, the block is summed from zero in tap order and added to the output's accumulator.  Chunks whose
// taps meet no sample of the tile are skipped (they would add zeros).  Two roles: `store` writes y, `energy` (the early part) writes
// one double per tile - the sum of its outputs squared by a fixed tree.  What bounds it: AUG_R * XV_AUG_KB fmas per lane and block
// against ~(AUG_R + 2 XV_AUG_KB) / 4 16-byte LDS reads - the vector ALU, with the LDS at about half its rate; HBM sees 2 bytes per
// staged sample.
// aug_power_kernel / aug_mix_kernel / aug_finish_kernel: the double sums in fixed orders, the noises, steps 5 - 7.  No floating-point
// atomics (the clip count is an integer one): the bits depend on the shape of the call only.  gfx950 only.
#include <math.h>

#include "xv_common.h"
#include "xv_ew.h"

#define AUG_TILE XV_AUG_TILE
#define AUG_KB XV_AUG_KB
#define AUG_R 8                             // consecutive outputs per lane
#define AUG_THREADS (AUG_TILE / AUG_R)      // 128
#define AUG_KC 512                          // taps staged per chunk
#define AUG_PER (AUG_TILE / AUG_THREADS)    // samples per thread in mix / finish
#define AUG_POWER_THREADS 1024              // threads of the one workgroup that sums a signal's squares
static_assert(AUG_KC % AUG_KB == 0 && AUG_KB % 4 == 0 && AUG_R % 4 == 0 && AUG_THREADS % 64 == 0, "window reads start on 16 bytes");

struct AugUtt { long src_off, n, rir_off, L, es, ee, p, nz_first, nz_count, out_off; };
struct AugNoise { long off, len, snr_bits, start, span; };
static_assert(sizeof(AugUtt) == 8 * XV_AUG_UTT_WORDS && sizeof(AugNoise) == 8 * XV_AUG_NOISE_WORDS, "the table layout of the header");

struct AugParams {
    const AugUtt* utt;
    const AugNoise* noise;
    const long* tile;            // [n_tiles][2]
    const int16_t *src, *rir, *nz;
    float* y;                    // [n_tiles][AUG_TILE]
    double *part_e, *part_y;     // [n_tiles]
    double *p_src, *p_noise;     // [b], [n_entries]: sums of squares
    int b, shift_output, normalize;
    float volume;
};

// the sum of v over the N threads of the workgroup by a fixed tree; valid in thread 0
template <int N = AUG_THREADS>
__device__ __forceinline__ double aug_tree(double v, double* part) {
    static_assert((N & (N - 1)) == 0, "the tree halves");
    const int tid = threadIdx.x;
    part[tid] = v;
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    return part[0];
}

// the first tile of utterance u: its tiles are consecutive, and the tile in hand (g, first output t0) is one of them
__device__ __forceinline__ long aug_tile0(long g, long t0) { return g - t0 / AUG_TILE; }

template <bool ENERGY>
__global__ __launch_bounds__(AUG_THREADS) void aug_fir_kernel(AugParams P) {
    XV_EW_PRIORITY();
    __shared__ __attribute__((aligned(16))) float xs[AUG_TILE + AUG_KC];
    __shared__ __attribute__((aligned(16))) float hs[AUG_KC];
    __shared__ double part[AUG_THREADS];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const AugUtt u = P.utt[P.tile[2 * g]];
    const long t0 = P.tile[2 * g + 1];
    if (u.rir_off < 0) return;
    const long n = u.n, L = ENERGY ? u.ee - u.es : u.L, M = n + L - 1;
    if (t0 >= M) return;      // uniform: the early convolution is shorter than y
    const int16_t* x = P.src + u.src_off;
    const int16_t* h = P.rir + u.rir_off + (ENERGY ? u.es : 0);
    // taps that meet a sample of this tile: k in [max(0, t0 - n + 1), min(L, t0 + AUG_TILE))
    const long k_lo = max(t0 - n + 1, 0L) / AUG_KC * AUG_KC, k_hi = min(L, t0 + AUG_TILE);
    float acc[AUG_R];
#pragma unroll
    for (int r = 0; r < AUG_R; ++r) acc[r] = 0.f;
#pragma unroll 1
    for (long kc0 = k_lo; kc0 < k_hi; kc0 += AUG_KC) {
        __syncthreads();
        const long base = t0 - kc0 - (AUG_KC - 1);      // xs[j] = x[base + j]
        for (int j = tid; j < AUG_TILE + AUG_KC; j += AUG_THREADS) {
            const long q = base + j;
            xs[j] = (q >= 0 && q < n) ? (float)x[q] : 0.f;
        }
        for (int j = tid; j < AUG_KC; j += AUG_THREADS) hs[j] = kc0 + j < L ? (float)h[kc0 + j] : 0.f;
        __syncthreads();
#pragma unroll 1
        for (int kb = 0; kb < AUG_KC && kc0 + kb < k_hi; kb += AUG_KB) {
            // output o = t0 + tid * AUG_R + r meets tap kc0 + kb + kk at xs[tid * AUG_R + r - kb - kk + AUG_KC - 1] = w[r - kk + AUG_KB - 1]
            float w[AUG_R + AUG_KB - 1], blk[AUG_R];
            const float* win = xs + tid * AUG_R + (AUG_KC - kb - AUG_KB);
#pragma unroll
            for (int m = 0; m < AUG_R + AUG_KB - 1; ++m) w[m] = win[m];
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) blk[r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < AUG_KB; ++kk) {
                const float tap = hs[kb + kk];
#pragma unroll
                for (int r = 0; r < AUG_R; ++r) blk[r] = fmaf(tap, w[r - kk + AUG_KB - 1], blk[r]);
            }
#pragma unroll
            for (int r = 0; r < AUG_R; ++r) acc[r] += blk[r];
        }
    }
    const long o0 = t0 + (long)tid * AUG_R;
    if (ENERGY) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < AUG_R; ++r)
            if (o0 + r < M) s += (double)acc[r] * (double)acc[r];
        s = aug_tree(s, part);
        if (tid == 0) P.part_e[g] = s;
    } else {
        float* y = P.y + g * AUG_TILE + tid * AUG_R;
#pragma unroll
        for (int r = 0; r < AUG_R; ++r)
            if (o0 + r < M) y[r] = acc[r];
    }
}

// Sums of squares in double: workgroup s < b the source of utterance s, workgroup b + e the span of noise entry e.  Thread k adds the
// samples k, k + AUG_POWER_THREADS, ... (the pattern of xv_energy_vad's column sum, 1024 threads wide: a 20 s signal is 313 dependent
// adds per thread), a fixed tree adds the partials.  The index into a repeated noise wraps by a compare and a subtract - no division per
// sample; lengths are below 2^31, so idx + step < 2^32.
__global__ __launch_bounds__(AUG_POWER_THREADS) void aug_power_kernel(AugParams P) {
    XV_EW_PRIORITY();
    __shared__ double part[AUG_POWER_THREADS];
    const int tid = threadIdx.x;
    const long s = blockIdx.x;
    const int16_t* v;
    long len, span;
    if (s < P.b) {
        v = P.src + P.utt[s].src_off;
        len = span = P.utt[s].n;
    } else {
        const AugNoise e = P.noise[s - P.b];
        v = P.nz + e.off;
        len = e.len;
        span = e.span;
    }
    const unsigned ulen = (unsigned)len, step = (unsigned)(AUG_POWER_THREADS % len);
    unsigned idx = (unsigned)(tid % len);      // = i mod len throughout
    double sum = 0.0;
    for (long i = tid; i < span; i += AUG_POWER_THREADS) {
        const double a = (double)v[idx];
        sum += a * a;
        idx += step;
        if (idx >= ulen) idx -= ulen;
    }
    sum = aug_tree<AUG_POWER_THREADS>(sum, part);
    if (tid == 0) (s < P.b ? P.p_src[s] : P.p_noise[s - P.b]) = sum;
}

// Step 4 on one tile: y = x where there is no impulse response, then the noises in list order, one fma per sample and noise; writes y and
// the tile's sum of y^2.  E is the sum of the early partials in index order, formed by every thread alike.
__global__ __launch_bounds__(AUG_THREADS) void aug_mix_kernel(AugParams P) {
    XV_EW_PRIORITY();
    __shared__ double part[AUG_THREADS];
    const int tid = threadIdx.x;
    const long g = blockIdx.x, ui = P.tile[2 * g], t0 = P.tile[2 * g + 1];
    const AugUtt u = P.utt[ui];
    const bool rir = u.rir_off >= 0;
    const long n = u.n, M = rir ? n + u.L - 1 : n;
    float* y = P.y + g * AUG_TILE;
    float v[AUG_PER];
#pragma unroll
    for (int j = 0; j < AUG_PER; ++j) {
        const long i = t0 + tid + j * AUG_THREADS;
        v[j] = 0.f;
        if (i < M) v[j] = rir ? y[tid + j * AUG_THREADS] : (float)P.src[u.src_off + i];
    }
    double E;
    if (rir) {
        const long me = n + (u.ee - u.es) - 1, tiles = (me + AUG_TILE - 1) / AUG_TILE, g0 = aug_tile0(g, t0);
        E = 0.0;
        for (long k = 0; k < tiles; ++k) E += P.part_e[g0 + k];
        E /= (double)me;
    } else {
        E = P.p_src[ui] / (double)n;
    }
    for (long e = u.nz_first; e < u.nz_first + u.nz_count; ++e) {
        const AugNoise z = P.noise[e];
        const double pn = P.p_noise[e] / (double)z.span;
        if (!(pn > 0.0) || z.start >= M) continue;      // uniform
        const float gain = (float)sqrt(pow(10.0, -(double)__int_as_float((int)z.snr_bits) / 10.0) * E / pn);
        const long end = z.start + min(z.span, M - z.start);
        const int16_t* nz = P.nz + z.off;
#pragma unroll
        for (int j = 0; j < AUG_PER; ++j) {
            const long i = t0 + tid + j * AUG_THREADS;
            if (i >= z.start && i < end) v[j] = fmaf(gain, (float)nz[(unsigned)(i - z.start) % (unsigned)z.len], v[j]);
        }
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < AUG_PER; ++j) {
        const long i = t0 + tid + j * AUG_THREADS;
        if (i < M) {
            y[tid + j * AUG_THREADS] = v[j];
            s += (double)v[j] * (double)v[j];
        }
    }
    s = aug_tree(s, part);
    if (tid == 0) P.part_y[g] = s;
}

// Steps 5 - 7 on the outputs [t0, t0 + AUG_TILE) of an utterance.  Pa is the sum of the mix partials in index order.
__global__ __launch_bounds__(AUG_THREADS) void aug_finish_kernel(AugParams P, int16_t* __restrict__ out_pcm, float* __restrict__ out_f32,
                                                                 int* __restrict__ out_samples, int* __restrict__ clipped) {
    XV_EW_PRIORITY();
    __shared__ int count[AUG_THREADS];
    const int tid = threadIdx.x;
    const long g = blockIdx.x, ui = P.tile[2 * g], t0 = P.tile[2 * g + 1];
    const AugUtt u = P.utt[ui];
    const bool rir = u.rir_off >= 0;
    const long n = u.n, M = rir ? n + u.L - 1 : n;
    const long n_out = P.shift_output ? n : M, shift = P.shift_output && rir ? u.p : 0;
    if (t0 == 0 && tid == 0) out_samples[ui] = (int)n_out;
    if (t0 >= n_out) return;      // uniform
    const long tiles = (M + AUG_TILE - 1) / AUG_TILE, g0 = aug_tile0(g, t0);
    double pa = 0.0;
    for (long k = 0; k < tiles; ++k) pa += P.part_y[g0 + k];
    pa /= (double)M;
    double sd = 1.0;
    if (P.normalize && pa > 0.0) sd = sqrt(P.p_src[ui] / (double)n / pa);
    if (P.volume > 0.f) sd *= (double)P.volume;
    const float scale = (float)sd;
    const float* y = P.y + g0 * AUG_TILE;      // the utterance's y: tile after tile, so sample i is y[i]
    int changed = 0;
#pragma unroll
    for (int j = 0; j < AUG_PER; ++j) {
        const long i = t0 + tid + j * AUG_THREADS;
        if (i < n_out) {
            long q = i + shift;      // (i + shift) mod M: i < n_out <= M and shift < M, so one subtraction folds it
            if (q >= M) q -= M;
            const float val = y[q] * scale;
            const float t = truncf(val), c = fminf(fmaxf(t, -32768.f), 32767.f);
            changed += c != t;
            out_pcm[u.out_off + i] = (int16_t)c;
            if (out_f32) out_f32[u.out_off + i] = val;
        }
    }
    count[tid] = changed;
    __syncthreads();
    for (int o = AUG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) count[tid] += count[tid + o];
        __syncthreads();
    }
    if (tid == 0 && count[0]) atomicAdd(clipped + ui, count[0]);      // an integer count: its value does not depend on the order
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
extern "C" int xv_debug_augment_plan(int64_t n, int64_t L, int out[4]) {
    XV_REQUIRE(out, "augment_plan: no output");
    XV_REQUIRE(n >= 1 && L >= 0 && n + L < (1L << 31), "augment_plan: n >= 1, L >= 0 (0: no impulse response) and n + L < 2^31 are needed (got %ld, %ld)",
               (long)n, (long)L);
    const long M = L > 0 ? n + L - 1 : n;
    out[0] = (int)((M + AUG_TILE - 1) / AUG_TILE);
    out[1] = AUG_TILE;
    out[2] = AUG_KB;
    out[3] = L > 0 ? (int)(AUG_KB + (L + AUG_KB - 1) / AUG_KB) : 0;
    return 0;
}

struct AugLayout { size_t y, part_e, part_y, p_src, p_noise, total; };

static AugLayout aug_layout(int b, int n_entries, int64_t n_tiles) {
    AugLayout l;
    l.y = 0;
    l.part_e = xv_align((size_t)n_tiles * AUG_TILE * sizeof(float), 16);
    l.part_y = l.part_e + (size_t)n_tiles * sizeof(double);
    l.p_src = l.part_y + (size_t)n_tiles * sizeof(double);
    l.p_noise = l.p_src + (size_t)b * sizeof(double);
    l.total = xv_align(l.p_noise + (size_t)n_entries * sizeof(double), 16);
    return l;
}

extern "C" size_t xv_augment_workspace_bytes(int b, int n_entries, int64_t n_tiles) {
    if (b < 0 || n_entries < 0 || n_tiles < 0) return 0;
    return aug_layout(b, n_entries, n_tiles).total;
}

extern "C" int xv_augment(void* stream, const xv_augment_config* cfg, int b, int n_entries, int64_t n_tiles, const int16_t* src_pcm,
                          const int16_t* rir_pcm, const int16_t* noise_pcm, const int64_t* tables, size_t table_words, int any_rir, void* ws,
                          size_t ws_bytes, int16_t* out_pcm, float* out_f32, int32_t* out_samples, int32_t* clipped) {
    XV_REQUIRE(cfg, "augment: no configuration");
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_augment_config), "augment: xv_augment_config.struct_bytes is %d, this library's struct has %zu bytes",
               cfg->struct_bytes, sizeof(xv_augment_config));
    XV_REQUIRE(cfg->sample_frequency > 0.f && cfg->sample_frequency <= 1e6f, "augment: sample_frequency must be positive (got %g)", cfg->sample_frequency);
    XV_REQUIRE(cfg->volume >= 0.f && cfg->volume <= 1e6f, "augment: volume must lie in 0 (none) .. 1e6 (got %g)", cfg->volume);
    XV_REQUIRE(src_pcm && tables && ws && out_pcm && out_samples && clipped && b > 0 && n_entries >= 0, "augment: bad arguments");
    XV_REQUIRE(n_tiles >= b && n_tiles < (1L << 31) / 2, "augment: the tiles of a call must number %d (one per utterance) .. 2^30 (got %ld)", b, (long)n_tiles);
    XV_REQUIRE(!any_rir || rir_pcm, "augment: an utterance has an impulse response, but there is no pool of them");
    XV_REQUIRE(n_entries == 0 || noise_pcm, "augment: %d noise entries, but there is no pool of noises", n_entries);
    const size_t words = (size_t)XV_AUG_UTT_WORDS * b + (size_t)XV_AUG_NOISE_WORDS * n_entries + 2 * (size_t)n_tiles;
    XV_REQUIRE(table_words == words, "augment: the tables of %d utterances, %d noise entries and %ld tiles hold %zu words (got %zu)", b, n_entries,
               (long)n_tiles, words, table_words);
    const AugLayout l = aug_layout(b, n_entries, n_tiles);
    XV_REQUIRE(ws_bytes >= l.total && (uintptr_t)ws % 16 == 0, "augment: a 16-byte aligned workspace of %zu bytes is needed (xv_augment_workspace_bytes), got %zu",
               l.total, ws_bytes);
    static_assert(sizeof(long) == sizeof(int64_t), "the tables are read as long");
    AugParams P;
    P.utt = (const AugUtt*)tables;
    P.noise = (const AugNoise*)(tables + (size_t)XV_AUG_UTT_WORDS * b);
    P.tile = (const long*)(tables + (size_t)XV_AUG_UTT_WORDS * b + (size_t)XV_AUG_NOISE_WORDS * n_entries);
    P.src = src_pcm; P.rir = rir_pcm; P.nz = noise_pcm;
    char* w = (char*)ws;
    P.y = (float*)(w + l.y);
    P.part_e = (double*)(w + l.part_e); P.part_y = (double*)(w + l.part_y);
    P.p_src = (double*)(w + l.p_src); P.p_noise = (double*)(w + l.p_noise);
    P.b = b; P.shift_output = cfg->shift_output != 0; P.normalize = cfg->normalize_output != 0;
    P.volume = cfg->volume;
    hipStream_t s = (hipStream_t)stream;
    XV_CHECK_HIP(hipMemsetAsync(clipped, 0, (size_t)b * sizeof(int32_t), s));
    hipLaunchKernelGGL(aug_power_kernel, dim3(b + n_entries), dim3(AUG_POWER_THREADS), 0, s, P);
    if (any_rir) {
        hipLaunchKernelGGL(aug_fir_kernel<true>, dim3((unsigned)n_tiles), dim3(AUG_THREADS), 0, s, P);
        hipLaunchKernelGGL(aug_fir_kernel<false>, dim3((unsigned)n_tiles), dim3(AUG_THREADS), 0, s, P);
    }
    hipLaunchKernelGGL(aug_mix_kernel, dim3((unsigned)n_tiles), dim3(AUG_THREADS), 0, s, P);
    hipLaunchKernelGGL(aug_finish_kernel, dim3((unsigned)n_tiles), dim3(AUG_THREADS), 0, s, P, out_pcm, out_f32, (int*)out_samples, (int*)clipped);
    XV_LAUNCH_CHECK();
    return 0;
}
