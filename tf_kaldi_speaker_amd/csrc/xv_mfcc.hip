// MFCC features and the energy VAD from waveforms - what compute-mfcc-feats (--dither=0) and compute-vad-decision do in front of everything
// else in the recipe (egs/voxceleb/v1/run.sh:59-63).  Kaldi is not available where this project is built and tested: parity is BY
// RESTATEMENT.  include/xvector_hip.h states the arithmetic, tests/mfcc_ref.py restates it in fp64 NumPy, the kernels are held against that.
//
// xv_mfcc: one wave per frame, four waves to a workgroup, each walking MF_ITERS frames behind one copy of the constant tables into LDS.
// A lane gathers the samples lane, lane + 64, ... of its frame (reflected at the utterance's ends) from int16 into registers; the DC sum
// and the energy are wave butterflies (wave_sum, as in xv_rowsum.h); the N-point real FFT is an N/2-point complex radix-2 FFT in the
// wave's LDS slice (bit-reversed store, log2(N/2) stages) plus the split step; a lane per mel bin sums its triangle over the power
// spectrum, a lane per coefficient its DCT row - both serial, in index order.  What bounds it: per frame the kernel reads 2 S bytes of new
// samples and writes 4 num_ceps bytes, against roughly (N/4) log2(N/2) butterflies and a few thousand LDS accesses - LDS traffic and
// issue rate, not HBM.  Precise logf only; no fast-math intrinsics, no atomics: the bits depend on the shape of the call only.
// xv_fbank (compute-fbank-feats, --dither=0) is the same program stopped in front of the DCT: mf_kernel<N, EPI> runs ONE frame body
// (gather, DC, energy, pre-emphasis, window, FFT, spectrum; mf_mel_sum: a bin's triangle) under two epilogues - MF_MFCC keeps the
// log-mel energies in LDS and a lane per coefficient sums its DCT row, MF_FBANK stores the (log-)mel energies as they leave the sums, behind
// the log-energy column when use_energy asks for it, and hands the log-energy of every frame to energy_out, the column xv_energy_vad reads
// (d = 1): an fbank system gets its VAD decisions without a second feature pass.  Its tables are xv_mfcc's without the dct block.
// xv_energy_vad: one workgroup per utterance; column 0 summed in double in a fixed order, then one thread per frame counts its window.
// gfx950 only.
#include <float.h>
#include <math.h>

#include <vector>

#include "xv_common.h"
#include "xv_ew.h"

#define MF_WAVES 4            // waves (frames in flight) per workgroup of 256
#define MF_ITERS 4            // frames a wave walks: the tables reach LDS once per MF_WAVES * MF_ITERS frames
#define MF_MAX_BINS 128
#define VAD_THREADS 256

// ---- host: sizes and tables --------------------------------------------------------------------------------------------------------
// what xv_mfcc_config and xv_fbank_config share, under the name the messages carry; ceps == 0: no DCT (fbank)
struct MfSpec {
    const char* who;
    float sf, length_ms, shift_ms, lo, hi, preemph, lifter, energy_floor;
    int bins, ceps;
};

struct MfccDims {
    int L, S, N, bins, ceps;
    int off_tw, off_idx, off_w, off_dct, n_w, total;      // offsets in floats (the window is at 0)
    double sf, lo, hi;
};

static double mf_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

// first FFT bin, count and (w != nullptr) the weights of mel bin m
static void mf_mel_bin(const MfccDims& d, int m, int* first, int* count, double* w) {
    const double mlo = mf_mel(d.lo), delta = (mf_mel(d.hi) - mlo) / (d.bins + 1);
    const double left = mlo + m * delta, centre = mlo + (m + 1) * delta, right = mlo + (m + 2) * delta;
    int f0 = -1, f1 = -1;
    for (int k = 0; k < d.N / 2; ++k) {
        const double mel = mf_mel(k * d.sf / d.N);
        if (mel > left && mel < right) {
            if (f0 < 0) f0 = k;
            f1 = k;
            if (w) w[k - f0] = mel <= centre ? (mel - left) / (centre - left) : (right - mel) / (right - centre);
        }
    }
    *first = f0 < 0 ? 0 : f0;
    *count = f0 < 0 ? 0 : f1 - f0 + 1;
}

static int mf_spec_dims(const MfSpec& c, MfccDims* d) {
    XV_REQUIRE(c.sf > 0.f && c.sf <= 1e6f, "%s: sample_frequency must be positive (got %g)", c.who, c.sf);
    XV_REQUIRE(c.length_ms > 0.f && c.shift_ms > 0.f, "%s: frame_length_ms and frame_shift_ms must be positive (got %g, %g)", c.who, c.length_ms,
               c.shift_ms);
    d->sf = (double)c.sf;
    const double l = d->sf * 0.001 * (double)c.length_ms, s = d->sf * 0.001 * (double)c.shift_ms;
    XV_REQUIRE(l >= 2.0 && l <= 1024.0, "%s: frame_length_ms = %g is %g samples at %g Hz; the FFT sizes 128, 256, 512 and 1024 are supported "
               "(65 .. 1024 samples)", c.who, c.length_ms, l, d->sf);
    XV_REQUIRE(s >= 1.0 && s <= 1e6, "%s: frame_shift_ms = %g is %g samples at %g Hz; at least one is needed", c.who, c.shift_ms, s, d->sf);
    d->L = (int)l;
    d->S = (int)s;
    d->N = 1;
    while (d->N < d->L) d->N *= 2;
    XV_REQUIRE(d->N >= 128 && d->N <= 1024, "%s: frame_length_ms = %g is %d samples, an FFT of %d points; 128, 256, 512 and 1024 are supported",
               c.who, c.length_ms, d->L, d->N);
    d->bins = c.bins;
    d->ceps = c.ceps;
    XV_REQUIRE(d->bins >= 1 && d->bins <= MF_MAX_BINS, "%s: num_mel_bins must lie in 1 .. %d (got %d)", c.who, MF_MAX_BINS, d->bins);
    XV_REQUIRE(d->ceps >= 0 && d->ceps <= d->bins, "%s: num_ceps must lie in 1 .. num_mel_bins = %d (got %d)", c.who, d->bins, d->ceps);
    const double nyquist = 0.5 * d->sf;
    d->lo = (double)c.lo;
    d->hi = c.hi > 0.f ? (double)c.hi : nyquist + (double)c.hi;
    XV_REQUIRE(d->lo >= 0.0 && d->lo < nyquist, "%s: low_freq must lie in 0 .. the Nyquist frequency %g (got %g)", c.who, nyquist, d->lo);
    XV_REQUIRE(d->hi > d->lo && d->hi <= nyquist, "%s: high_freq = %g gives %g Hz; it must lie above low_freq = %g and not above the Nyquist frequency %g",
               c.who, c.hi, d->hi, d->lo, nyquist);
    XV_REQUIRE(c.preemph >= 0.f && c.preemph <= 1.f, "%s: preemphasis must lie in 0 .. 1 (got %g)", c.who, c.preemph);
    XV_REQUIRE(c.lifter >= 0.f, "%s: cepstral_lifter must not be negative (got %g)", c.who, c.lifter);
    XV_REQUIRE(c.energy_floor >= 0.f, "%s: energy_floor must not be negative (got %g)", c.who, c.energy_floor);
    d->n_w = 0;
    for (int m = 0; m < d->bins; ++m) {
        int first, count;
        mf_mel_bin(*d, m, &first, &count, nullptr);
        d->n_w += count;
    }
    d->off_tw = d->L;
    d->off_idx = d->off_tw + d->N;
    d->off_w = d->off_idx + 3 * d->bins;
    d->off_dct = d->off_w + d->n_w;
    d->total = d->off_dct + d->ceps * d->bins;
    return 0;
}

static int mf_dims(const xv_mfcc_config* c, MfccDims* d) {
    XV_REQUIRE(c, "mfcc: no configuration");
    XV_REQUIRE(c->struct_bytes == (int32_t)sizeof(xv_mfcc_config), "mfcc: xv_mfcc_config.struct_bytes is %d, this library's struct has %zu bytes",
               c->struct_bytes, sizeof(xv_mfcc_config));
    XV_REQUIRE(c->num_ceps >= 1, "mfcc: num_ceps must lie in 1 .. num_mel_bins = %d (got %d)", c->num_mel_bins, c->num_ceps);
    const MfSpec s = {"mfcc", c->sample_frequency, c->frame_length_ms, c->frame_shift_ms, c->low_freq, c->high_freq, c->preemphasis,
                      c->cepstral_lifter, c->energy_floor, c->num_mel_bins, c->num_ceps};
    return mf_spec_dims(s, d);
}

// the fbank tables are the MFCC ones without the dct block: ceps = 0 ends the layout at off_dct
static int fb_dims(const xv_fbank_config* c, MfccDims* d) {
    XV_REQUIRE(c, "fbank: no configuration");
    XV_REQUIRE(c->struct_bytes == (int32_t)sizeof(xv_fbank_config), "fbank: xv_fbank_config.struct_bytes is %d, this library's struct has %zu bytes",
               c->struct_bytes, sizeof(xv_fbank_config));
    const MfSpec s = {"fbank", c->sample_frequency, c->frame_length_ms, c->frame_shift_ms, c->low_freq, c->high_freq, c->preemphasis,
                      0.f, c->energy_floor, c->num_mel_bins, 0};
    if (int rc = mf_spec_dims(s, d)) return rc;
    const int cols = d->bins + (c->use_energy != 0);
    XV_REQUIRE(cols <= MF_MAX_BINS, "fbank: num_mel_bins = %d with use_energy gives %d columns; the front end and the 'CM ' encoder take at most %d",
               d->bins, cols, MF_MAX_BINS);
    return 0;
}

static long mf_frames(const MfccDims& d, int snip_edges, long n) {
    if (n <= 0) return 0;
    return snip_edges ? (n < d.L ? 0 : 1 + (n - d.L) / d.S) : (n + d.S / 2) / d.S;
}

// window, twiddles, mel_bins, mel_w: everything in front of the dct block
static void mf_front_tables(const MfccDims& d, float* h_out) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < d.L; ++i) h_out[i] = (float)pow(0.5 - 0.5 * cos(2.0 * pi * i / (d.L - 1)), 0.85);
    for (int k = 0; k < d.N / 2; ++k) {
        h_out[d.off_tw + 2 * k] = (float)cos(2.0 * pi * k / d.N);
        h_out[d.off_tw + 2 * k + 1] = (float)-sin(2.0 * pi * k / d.N);
    }
    std::vector<double> w(d.N / 2);
    int at = 0;
    for (int m = 0; m < d.bins; ++m) {
        int first, count;
        mf_mel_bin(d, m, &first, &count, w.data());
        h_out[d.off_idx + 3 * m] = (float)first;
        h_out[d.off_idx + 3 * m + 1] = (float)count;
        h_out[d.off_idx + 3 * m + 2] = (float)at;
        for (int j = 0; j < count; ++j) h_out[d.off_w + at + j] = (float)w[j];
        at += count;
    }
}

extern "C" int64_t xv_mfcc_num_frames(const xv_mfcc_config* cfg, int64_t samples) {
    MfccDims d;
    if (mf_dims(cfg, &d)) return -1;
    return mf_frames(d, cfg->snip_edges, (long)samples);
}

extern "C" size_t xv_mfcc_table_floats(const xv_mfcc_config* cfg) {
    MfccDims d;
    if (mf_dims(cfg, &d)) return 0;
    return (size_t)d.total;
}

extern "C" int xv_mfcc_tables(const xv_mfcc_config* cfg, float* h_out, size_t floats) {
    MfccDims d;
    if (int rc = mf_dims(cfg, &d)) return rc;
    XV_REQUIRE(h_out && floats == (size_t)d.total, "mfcc_tables: a host buffer of %d floats is needed (xv_mfcc_table_floats), got %zu", d.total, floats);
    mf_front_tables(d, h_out);
    const double pi = 3.14159265358979323846;
    const double q = (double)cfg->cepstral_lifter;
    for (int c = 0; c < d.ceps; ++c) {
        const double lift = q > 0.0 ? 1.0 + 0.5 * q * sin(pi * c / q) : 1.0;
        for (int m = 0; m < d.bins; ++m) {
            const double v = c == 0 ? sqrt(1.0 / d.bins) : sqrt(2.0 / d.bins) * cos(pi / d.bins * (m + 0.5) * c);
            h_out[d.off_dct + c * d.bins + m] = (float)(v * lift);
        }
    }
    return 0;
}

extern "C" int64_t xv_fbank_num_frames(const xv_fbank_config* cfg, int64_t samples) {
    MfccDims d;
    if (fb_dims(cfg, &d)) return -1;
    return mf_frames(d, cfg->snip_edges, (long)samples);
}

extern "C" size_t xv_fbank_table_floats(const xv_fbank_config* cfg) {
    MfccDims d;
    if (fb_dims(cfg, &d)) return 0;
    return (size_t)d.total;
}

extern "C" int xv_fbank_tables(const xv_fbank_config* cfg, float* h_out, size_t floats) {
    MfccDims d;
    if (int rc = fb_dims(cfg, &d)) return rc;
    XV_REQUIRE(h_out && floats == (size_t)d.total, "fbank_tables: a host buffer of %d floats is needed (xv_fbank_table_floats), got %zu", d.total, floats);
    mf_front_tables(d, h_out);
    return 0;
}

// ---- device ------------------------------------------------------------------------------------------------------------------------
struct MfccParams {
    int L, S, bins, ceps, off_tw, off_idx, off_w, off_dct, n_w, total, t_out;
    int snip_edges, remove_dc, use_energy, raw_energy;
    float preemph, log_energy_floor;      // the floor is -inf when there is none
    int d, use_log, use_power;            // d: floats per output row (num_ceps; fbank: bins + use_energy); use_log / use_power: fbank only
};

enum { MF_MFCC = 0, MF_FBANK = 1 };      // the epilogue of mf_kernel

// floats of a wave's LDS slice: the FFT buffer [N], the power spectrum [N/2] and, for the DCT, the log-mel energies [MF_MAX_BINS]
static constexpr int mf_slice_floats(int N, int epi) { return N + N / 2 + (epi == MF_MFCC ? MF_MAX_BINS : 0); }

// LDS of a workgroup, in floats: the tables (rounded up to 4), then a slice per wave
static inline size_t mf_lds_floats(int total, int N, int epi) { return xv_align(total, 4) + (size_t)MF_WAVES * mf_slice_floats(N, epi); }

// E[m]: bin m's triangle over P, serial, in index order
template <int N>
__device__ __forceinline__ float mf_mel_sum(const MfccParams& p,const float* midx, const float* mw, const float* P, int m) {
    constexpr int M = N / 2;
    int first = (int)midx[3 * m], cnt = (int)midx[3 * m + 1], off = (int)midx[3 * m + 2];
    first = min(max(first, 0), M - 1);      // a table that is not the library's own must not send a read outside LDS
    cnt = min(max(cnt, 0), M - first);
    off = min(max(off, 0), max(p.n_w - cnt, 0));
    cnt = min(cnt, p.n_w);
    float e = 0.f;
    for (int j = 0; j < cnt; ++j) e = fmaf(mw[off + j], P[first + j], e);
    return e;
}

// Both feature kinds: the frame body (gather, DC, energy, pre-emphasis, window, FFT, spectrum) stands here once, the two epilogues behind
// it.  The body is kept in the kernel, not in a device function of its own: hoisted out, the N = 512 and 1024 instantiations took 78 and
// 264 VGPRs instead of 64 and 92 (the compiler then schedules the gathers of all PER samples together).
template <int N, int EPI>
__global__ __launch_bounds__(64 * MF_WAVES) void mf_kernel(MfccParams p, const float* __restrict__ tables, const int16_t* __restrict__ pcm,
                                                          const long* __restrict__ offsets, const int* __restrict__ samples,
                                                          float* __restrict__ out, int* __restrict__ rows_out, float* __restrict__ energy_out) {
    XV_EW_PRIORITY();
    constexpr int M = N / 2, PER = N / XV_WAVE, LOG2M = N == 128 ? 6 : N == 256 ? 7 : N == 512 ? 8 : 9, SLICE = mf_slice_floats(N, EPI);
    static_assert(N == 128 || N == 256 || N == 512 || N == 1024, "four FFT sizes");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & (XV_WAVE - 1), wave = tid / XV_WAVE, i = blockIdx.y;
    const long n = samples[i];
    long T = 0;
    if (n > 0) T = p.snip_edges ? (n < p.L ? 0 : 1 + (n - p.L) / p.S) : (n + p.S / 2) / p.S;
    const int rows = (int)(T < (long)p.t_out ? T : (long)p.t_out);
    if (blockIdx.x == 0 && tid == 0) rows_out[i] = rows;
    const int f_first = blockIdx.x * (MF_WAVES * MF_ITERS);
    float* oi = out + (long)i * p.t_out * p.d;
    float* ei = EPI == MF_FBANK && energy_out ? energy_out + (long)i * p.t_out : nullptr;
    if (f_first >= rows) {      // uniform: nothing but padding rows in this workgroup
        const int f_end = min(f_first + MF_WAVES * MF_ITERS, p.t_out);
        for (int e = f_first * p.d + tid; e < f_end * p.d; e += 64 * MF_WAVES) oi[e] = 0.f;
        if (ei)
            for (int f = f_first + tid; f < f_end; f += 64 * MF_WAVES) ei[f] = 0.f;
        return;
    }
    for (int e = tid; e < p.total; e += 64 * MF_WAVES) lds[e] = tables[e];
    const float* win = lds;
    const float* tw = lds + p.off_tw;
    const float* midx = lds + p.off_idx;
    const float* mw = lds + p.off_w;
    float* buf = lds + ((p.total + 3) & ~3) + wave * SLICE;
    float* P = buf + N;
    const int16_t* x = pcm + offsets[i];
    __syncthreads();
    for (int it = 0; it < MF_ITERS; ++it) {
        const int f = f_first + it * MF_WAVES + wave;
        if (f_first + it * MF_WAVES >= p.t_out) break;      // uniform
        const bool valid = f < rows;                          // per wave; an invalid wave runs on zeros and keeps the barriers
        float v[PER];
        const long start = p.snip_edges ? (long)f * p.S : (long)p.S * f + p.S / 2 - p.L / 2;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int idx = lane + XV_WAVE * j;
            v[j] = 0.f;
            if (valid && idx < p.L) {
                long q = start + idx;
                while (q < 0 || q >= n) q = q < 0 ? -q - 1 : 2 * n - 1 - q;
                v[j] = (float)x[q];
            }
        }
        if (p.remove_dc) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < PER; ++j) sum += v[j];
            const float mean = wave_sum(sum) / (float)p.L;
#pragma unroll
            for (int j = 0; j < PER; ++j)
                if (lane + XV_WAVE * j < p.L) v[j] -= mean;
        }
        float log_e = 0.f;
        if (p.raw_energy) {
            float e = 0.f;
#pragma unroll
            for (int j = 0; j < PER; ++j) e = fmaf(v[j], v[j], e);
            log_e = logf(fmaxf(wave_sum(e), FLT_EPSILON));
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) buf[lane + XV_WAVE * j] = v[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {      // pre-emphasis (every sample minus p times the one in front, the first minus p times itself), window
            const int idx = lane + XV_WAVE * j;
            v[j] = idx < p.L ? (v[j] - p.preemph * buf[idx > 0 ? idx - 1 : 0]) * win[idx] : 0.f;
        }
        if (!p.raw_energy) {
            float e = 0.f;
#pragma unroll
            for (int j = 0; j < PER; ++j) e = fmaf(v[j], v[j], e);
            log_e = logf(fmaxf(wave_sum(e), FLT_EPSILON));
        }
        __syncthreads();
        // z[k] = (w[2k], w[2k + 1]) stored at the bit-reversed k: the radix-2 stages below then run in place
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int idx = lane + XV_WAVE * j;
            const int r = (int)(__brev((unsigned)(idx >> 1)) >> (32 - LOG2M));
            buf[2 * r + (idx & 1)] = v[j];
        }
        __syncthreads();
#pragma unroll 1
        for (int half = 1; half < M; half <<= 1) {
            const int tstep = M / half;      // W_M^(pos M / (2 half)) = W_N^(pos M / half)
            for (int bf = lane; bf < M / 2; bf += XV_WAVE) {
                const int pos = bf & (half - 1), i0 = ((bf - pos) << 1) + pos, i1 = i0 + half;
                const float wr = tw[2 * pos * tstep], wi = tw[2 * pos * tstep + 1];
                const float ar = buf[2 * i0], ai = buf[2 * i0 + 1], br = buf[2 * i1], bi = buf[2 * i1 + 1];
                const float tr = br * wr - bi * wi, ti = br * wi + bi * wr;
                buf[2 * i0] = ar + tr; buf[2 * i0 + 1] = ai + ti;
                buf[2 * i1] = ar - tr; buf[2 * i1 + 1] = ai - ti;
            }
            __syncthreads();
        }
        // split step: X[k] = A - i W_N^k B, A = (Z[k] + conj Z[M - k]) / 2, B = (Z[k] - conj Z[M - k]) / 2
        for (int k = lane; k < M; k += XV_WAVE) {
            const int km = (M - k) & (M - 1);
            const float zr = buf[2 * k], zi = buf[2 * k + 1], mr = buf[2 * km], mi = buf[2 * km + 1];
            const float ar = 0.5f * (zr + mr), ai = 0.5f * (zi - mi), br = 0.5f * (zr - mr), bi = 0.5f * (zi + mi);
            const float wr = tw[2 * k], wi = tw[2 * k + 1];
            const float xr = ar + (wr * bi + wi * br), xi = ai - (wr * br - wi * bi);
            const float pw = xr * xr + xi * xi;
            P[k] = EPI == MF_FBANK && !p.use_power ? sqrtf(pw) : pw;
        }
        __syncthreads();
        if (EPI == MF_MFCC) {
            const float* dct = lds + p.off_dct;
            float* lm = P + N / 2;
            for (int m = lane; m < p.bins; m += XV_WAVE) lm[m] = logf(fmaxf(mf_mel_sum<N>(p, midx, mw, P, m), FLT_EPSILON));
            __syncthreads();
            for (int c = lane; c < p.ceps; c += XV_WAVE) {
                const float* row = dct + c * p.bins;
                float acc = 0.f;
                for (int m = 0; m < p.bins; ++m) acc = fmaf(row[m], lm[m], acc);
                if (c == 0 && p.use_energy) acc = fmaxf(log_e, p.log_energy_floor);
                if (f < p.t_out) oi[(long)f * p.ceps + c] = valid ? acc : 0.f;
            }
        } else {
            for (int m = lane; m < p.bins; m += XV_WAVE) {
                const float e = mf_mel_sum<N>(p, midx, mw, P, m);
                const float col = p.use_log ? logf(fmaxf(e, FLT_EPSILON)) : e;
                if (f < p.t_out) oi[(long)f * p.d + p.use_energy + m] = valid ? col : 0.f;
            }
            if (lane == 0 && f < p.t_out) {
                const float e0 = valid ? fmaxf(log_e, p.log_energy_floor) : 0.f;
                if (p.use_energy) oi[(long)f * p.d] = e0;
                if (ei) ei[f] = e0;
            }
        }
    }
}

// the launch of both entry points: p holds the options, d the sizes of the tables at tables_dev
template <int EPI>
static int mf_launch(hipStream_t s, const MfccDims& d, MfccParams p, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
                     const int32_t* samples, int b, int t_out, float* out, int32_t* rows_out, float* energy_out) {
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    p.L = d.L; p.S = d.S; p.bins = d.bins; p.ceps = d.ceps;
    p.off_tw = d.off_tw; p.off_idx = d.off_idx; p.off_w = d.off_w; p.off_dct = d.off_dct; p.n_w = d.n_w; p.total = d.total;
    p.t_out = t_out;
    const size_t lds_bytes = mf_lds_floats(d.total, d.N, EPI) * sizeof(float);
    dim3 grid(xv_cdiv(t_out, MF_WAVES * MF_ITERS), b);
#define MF_LAUNCH(NN)                                                                                                               \
    do {                                                                                                                            \
        if (lds_bytes > 64 * 1024)                                                                                                  \
            XV_CHECK_HIP(hipFuncSetAttribute((const void*)mf_kernel<NN, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes)); \
        hipLaunchKernelGGL((mf_kernel<NN, EPI>), grid, dim3(64 * MF_WAVES), lds_bytes, s, p, tables_dev, pcm, (const long*)offsets,  \
                           (const int*)samples, out, (int*)rows_out, energy_out);                                                   \
    } while (0)
    switch (d.N) {
        case 128: MF_LAUNCH(128); break;
        case 256: MF_LAUNCH(256); break;
        case 512: MF_LAUNCH(512); break;
        default: MF_LAUNCH(1024); break;
    }
#undef MF_LAUNCH
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_mfcc(void* stream, const xv_mfcc_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
                       const int32_t* samples, int b, int t_out, float* out, int32_t* rows_out) {
    MfccDims d;
    if (int rc = mf_dims(cfg, &d)) return rc;
    XV_REQUIRE(tables_dev && pcm && offsets && samples && out && rows_out && b > 0 && t_out > 0, "mfcc: bad arguments");
    XV_REQUIRE(b <= 65535, "mfcc: at most 65535 utterances a call (got %d)", b);
    XV_REQUIRE((long)t_out * d.ceps < (1L << 31), "mfcc: t_out * num_ceps must stay below 2^31 (got %d * %d)", t_out, d.ceps);
    MfccParams p;
    p.snip_edges = cfg->snip_edges != 0; p.remove_dc = cfg->remove_dc_offset != 0;
    p.use_energy = cfg->use_energy != 0; p.raw_energy = cfg->raw_energy != 0;
    p.preemph = cfg->preemphasis;
    p.log_energy_floor = cfg->energy_floor > 0.f ? logf(cfg->energy_floor) : -INFINITY;
    p.d = d.ceps; p.use_log = 1; p.use_power = 1;
    return mf_launch<MF_MFCC>((hipStream_t)stream, d, p, tables_dev, pcm, offsets, samples, b, t_out, out, rows_out, nullptr);
}

extern "C" int xv_fbank(void* stream, const xv_fbank_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
                        const int32_t* samples, int b, int t_out, float* out, int32_t* rows_out, float* energy_out) {
    MfccDims d;
    if (int rc = fb_dims(cfg, &d)) return rc;
    XV_REQUIRE(tables_dev && pcm && offsets && samples && out && rows_out && b > 0 && t_out > 0, "fbank: bad arguments");
    XV_REQUIRE(b <= 65535, "fbank: at most 65535 utterances a call (got %d)", b);
    MfccParams p;
    p.snip_edges = cfg->snip_edges != 0; p.remove_dc = cfg->remove_dc_offset != 0;
    p.use_energy = cfg->use_energy != 0; p.raw_energy = cfg->raw_energy != 0;
    p.preemph = cfg->preemphasis;
    p.log_energy_floor = cfg->energy_floor > 0.f ? logf(cfg->energy_floor) : -INFINITY;
    p.d = d.bins + p.use_energy; p.use_log = cfg->use_log_fbank != 0; p.use_power = cfg->use_power != 0;
    XV_REQUIRE((long)t_out * p.d < (1L << 31), "fbank: t_out * (num_mel_bins + use_energy) must stay below 2^31 (got %d * %d)", t_out, p.d);
    return mf_launch<MF_FBANK>((hipStream_t)stream, d, p, tables_dev, pcm, offsets, samples, b, t_out, out, rows_out, energy_out);
}

// masks[i][f] for f < t: the decision of frame f of piece i, 0 behind its rows.  The column sum: thread k adds the frames k, k + 256, ... in
// double, a fixed tree in LDS adds the 256 partials.
__global__ __launch_bounds__(VAD_THREADS) void energy_vad_kernel(const float* __restrict__ x, const int* __restrict__ rows, int t, int d, float threshold,
                                                                 float mean_scale, int context, float proportion, uint8_t* __restrict__ masks) {
    XV_EW_PRIORITY();
    __shared__ double part[VAD_THREADS];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(rows[i], 0), t);
    const float* e = x + (long)i * t * d;
    uint8_t* mi = masks + (long)i * t;
    double thr = (double)threshold;
    if (mean_scale != 0.f && n > 0) {
        double sum = 0.0;
        for (int f = tid; f < n; f += VAD_THREADS) sum += (double)e[(long)f * d];
        part[tid] = sum;
        __syncthreads();
        for (int o = VAD_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) part[tid] += part[tid + o];
            __syncthreads();
        }
        thr += (double)mean_scale * (part[0] / (double)n);
    }
    for (int f = tid; f < t; f += VAD_THREADS) {
        uint8_t voiced = 0;
        if (f < n) {
            const int lo = max(f - context, 0), hi = min(f + context, n - 1);
            int cnt = 0;
            for (int g = lo; g <= hi; ++g) cnt += (double)e[(long)g * d] > thr;
            voiced = (double)cnt >= (double)(hi - lo + 1) * (double)proportion;
        }
        mi[f] = voiced;
    }
}

extern "C" int xv_energy_vad(void* stream, const float* x, const int32_t* rows, int b, int t, int d, float threshold, float mean_scale,
                             int frames_context, float proportion, uint8_t* masks) {
    XV_REQUIRE(x && rows && masks && b > 0 && t > 0 && d > 0, "energy_vad: bad arguments");
    XV_REQUIRE(b <= (1 << 30), "energy_vad: at most 2^30 pieces a call (got %d)", b);
    XV_REQUIRE(frames_context >= 0 && frames_context <= (1 << 20), "energy_vad: frames_context must lie in 0 .. 2^20 (got %d)", frames_context);
    XV_REQUIRE(proportion > 0.f && proportion <= 1.f, "energy_vad: proportion must lie in (0, 1] (got %g)", proportion);
    hipLaunchKernelGGL(energy_vad_kernel, dim3(b), dim3(VAD_THREADS), 0, (hipStream_t)stream, x, (const int*)rows, t, d, threshold, mean_scale,
                       frames_context, proportion, masks);
    XV_LAUNCH_CHECK();
    return 0;
}
