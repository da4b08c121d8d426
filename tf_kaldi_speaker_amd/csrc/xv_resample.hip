// Sample-rate conversion of waveforms - what the `sox -r 8k` stages of the SRE recipe (egs/sre/v1/local/make_musan.sh, run.sh:135-142),
// compute-mfcc-feats --allow-downsample / --allow-upsample and the 0.9 / 1.1 speed perturbation of x-vector training do: a polyphase
// windowed-sinc FIR, Kaldi's LinearResample (feat/resample.{h,cc}) with ResampleWaveform's cutoff.  Kaldi is not available where this
// project is built and tested: parity is BY RESTATEMENT.  include/xvector_hip.h states the arithmetic, tests/resample_ref.py restates it
// in fp64, the kernel is held against that.
//
// resample_kernel: one launch, grid (tiles walked, utterances).  A workgroup copies the table into LDS once - the weight rows on an ODD
// pitch, so that the 32 lanes of a ds_read_b32 group, which own consecutive outputs = consecutive phases, read column j of 32 rows from
// 32 banks - and then walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its utterance.  Per tile of `tile` consecutive outputs
// the input span is staged as fp32 (int16 -> fp32 once, zeros outside [0, n) written by the staging: the inner loop has no bounds test),
// a lane owns the outputs tid, tid + 256, ... of the tile and sums each as ONE sequential fmaf chain from zero in increasing j over the
// taps_max columns of its row (the padding columns hold zeros and add nothing).  The bits of an output depend on x and the table only -
// not on the tile, the batch or the grid.  No floating-point atomics (the clip count is an integer one), no cross-workgroup hand-over.
// Per fma the loop issues two 4-byte LDS reads (a weight, a sample): what bounds it is stated in DESIGN.md section 6f from the bench leg
// (profiles/resample_bench.txt), not here.  gfx950 only.
#include <math.h>

#include "xv_common.h"

#define RS_THREADS 256
#define RS_R 4                                // outputs per lane and tile at the most
#define RS_MAX_TABLE 16384                    // floats of weight rows
#define RS_LDS_BUDGET (128 * 1024)            // bytes of dynamic LDS a workgroup may take (the CU has 160 KiB)
#define RS_MAX_RATE (1 << 24)                 // whole numbers below it are exact as floats (first, taps)

// ---- host: sizes and tables --------------------------------------------------------------------------------------------------------
struct RsDims {
    int fin, fout, num_zeros, in_unit, out_unit, taps_max, first_min, first_max, pitch, tile, span;
    double cutoff, ww;
    size_t table_floats, lds_bytes;
};

static long rs_gcd(long a, long b) {
    while (b) {
        const long r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// first input index and number of taps of phase i
static void rs_phase(const RsDims& d, int i, long* first, long* taps) {
    const double t = i / (double)d.fout;
    const long lo = (long)ceil((t - d.ww) * d.fin), hi = (long)floor((t + d.ww) * d.fin);
    *first = lo;
    *taps = hi - lo + 1;
}

static double rs_weight(const RsDims& d, double delta) {
    const double pi = 3.14159265358979323846;
    const double window = fabs(delta) < d.ww ? 0.5 * (1.0 + cos(2.0 * pi * d.cutoff / d.num_zeros * delta)) : 0.0;
    const double filter = delta != 0.0 ? sin(2.0 * pi * d.cutoff * delta) / (pi * delta) : 2.0 * d.cutoff;
    return filter * window / d.fin;
}

// staged samples of a tile of `tile` outputs: the outputs of a tile sit in at most qr + 1 periods of out_unit
static long rs_span(const RsDims& d, int tile) {
    const long qr = ((long)d.out_unit - 1 + tile - 1) / d.out_unit;
    return qr * d.in_unit + (d.first_max - d.first_min) + d.taps_max;
}

static size_t rs_lds_bytes(const RsDims& d, long span) { return ((size_t)d.out_unit * d.pitch + (size_t)d.out_unit + (size_t)span) * sizeof(float); }

static int rs_dims(const xv_resample_config* c, RsDims* d) {
    XV_REQUIRE(c, "resample: no configuration");
    XV_REQUIRE(c->struct_bytes == (int32_t)sizeof(xv_resample_config), "resample: xv_resample_config.struct_bytes is %d, this library's struct has %zu bytes",
               c->struct_bytes, sizeof(xv_resample_config));
    XV_REQUIRE(c->fin >= 1 && c->fout >= 1 && c->fin < RS_MAX_RATE && c->fout < RS_MAX_RATE, "resample: the rates must lie in 1 .. 2^24 Hz (got %d -> %d)",
               c->fin, c->fout);
    XV_REQUIRE(c->fin != c->fout, "resample: fin == fout == %d Hz: there is nothing to resample (callers skip the call)", c->fin);
    d->fin = c->fin;
    d->fout = c->fout;
    d->num_zeros = c->num_zeros == 0 ? 6 : c->num_zeros;
    XV_REQUIRE(d->num_zeros >= 1 && d->num_zeros <= 64, "resample: num_zeros must lie in 1 .. 64, or be 0 for the default 6 (got %d)", c->num_zeros);
    const int low = c->fin < c->fout ? c->fin : c->fout;
    d->cutoff = c->cutoff == 0.f ? 0.99 * 0.5 * low : (double)c->cutoff;
    XV_REQUIRE(d->cutoff > 0.0 && d->cutoff <= 0.5 * low, "resample: cutoff must lie in (0, %g] Hz, half the lower rate, or be 0 for the default (got %g)",
               0.5 * low, (double)c->cutoff);
    const long g = rs_gcd(c->fin, c->fout);
    d->in_unit = (int)(c->fin / g);
    d->out_unit = (int)(c->fout / g);
    d->ww = d->num_zeros / (2.0 * d->cutoff);
    XV_REQUIRE(d->out_unit <= RS_MAX_TABLE, "resample: %d -> %d Hz has %d phases, a table of more than %d floats; it must fit LDS beside the staged samples",
               d->fin, d->fout, d->out_unit, RS_MAX_TABLE);
    long tmax = 0, fmin = 0, fmax = 0;
    for (int i = 0; i < d->out_unit; ++i) {
        long first, taps;
        rs_phase(*d, i, &first, &taps);
        if (i == 0 || taps > tmax) tmax = taps;
        if (i == 0 || first < fmin) fmin = first;
        if (i == 0 || first > fmax) fmax = first;
    }
    XV_REQUIRE(tmax >= 1 && (long)d->out_unit * tmax <= RS_MAX_TABLE, "resample: %d -> %d Hz needs a table of %d phases x %ld taps = %ld floats, more than %d; "
               "it must fit LDS beside the staged samples", d->fin, d->fout, d->out_unit, tmax, (long)d->out_unit * tmax, RS_MAX_TABLE);
    XV_REQUIRE(fmin > -RS_MAX_RATE && fmax < RS_MAX_RATE, "resample: %d -> %d Hz: a first index of %ld .. %ld is not exact as a float", d->fin, d->fout, fmin, fmax);
    d->taps_max = (int)tmax;
    d->first_min = (int)fmin;
    d->first_max = (int)fmax;
    d->pitch = d->taps_max | 1;
    d->table_floats = 2 * (size_t)d->out_unit + (size_t)d->out_unit * d->taps_max;
    d->tile = 0;
    for (int tile = RS_THREADS * RS_R; tile >= RS_THREADS; tile /= 2) {
        const long span = rs_span(*d, tile);
        if (rs_lds_bytes(*d, span) <= RS_LDS_BUDGET) {
            d->tile = tile;
            d->span = (int)span;
            break;
        }
    }
    XV_REQUIRE(d->tile > 0, "resample: %d -> %d Hz: the table and the %ld samples staged for %d outputs take %zu bytes of LDS, more than %d", d->fin, d->fout,
               rs_span(*d, RS_THREADS), RS_THREADS, rs_lds_bytes(*d, rs_span(*d, RS_THREADS)), RS_LDS_BUDGET);
    d->lds_bytes = rs_lds_bytes(*d, d->span);
    return 0;
}

extern "C" int64_t xv_resample_num_samples(const xv_resample_config* cfg, int64_t samples) {
    RsDims d;
    if (rs_dims(cfg, &d)) return -1;
    if (samples <= 0) return 0;
    if (samples >= (1L << 31)) {
        xv_set_error("resample_num_samples: fewer than 2^31 samples are expected (got %ld)", (long)samples);
        return -1;
    }
    return (samples * d.out_unit + d.in_unit - 1) / d.in_unit;
}

extern "C" size_t xv_resample_table_floats(const xv_resample_config* cfg) {
    RsDims d;
    if (rs_dims(cfg, &d)) return 0;
    return d.table_floats;
}

extern "C" int xv_resample_tables(const xv_resample_config* cfg, float* h_out, size_t floats) {
    RsDims d;
    if (int rc = rs_dims(cfg, &d)) return rc;
    XV_REQUIRE(h_out && floats == d.table_floats, "resample_tables: a host buffer of %zu floats is needed (xv_resample_table_floats), got %zu", d.table_floats,
               floats);
    float* w = h_out + 2 * (size_t)d.out_unit;
    for (int i = 0; i < d.out_unit; ++i) {
        long first, taps;
        rs_phase(d, i, &first, &taps);
        h_out[i] = (float)first;
        h_out[d.out_unit + i] = (float)taps;
        const double t = i / (double)d.fout;
        for (int j = 0; j < d.taps_max; ++j) w[(size_t)i * d.taps_max + j] = j < taps ? (float)rs_weight(d, (first + j) / (double)d.fin - t) : 0.f;
    }
    return 0;
}

extern "C" int xv_debug_resample_plan(const xv_resample_config* cfg, int out[6]) {
    XV_REQUIRE(out, "resample_plan: no output");
    RsDims d;
    if (int rc = rs_dims(cfg, &d)) return rc;
    out[0] = d.in_unit;
    out[1] = d.out_unit;
    out[2] = d.taps_max;
    out[3] = d.tile;
    out[4] = d.span;
    out[5] = (int)d.lds_bytes;
    return 0;
}

// ---- device ------------------------------------------------------------------------------------------------------------------------
struct RsParams {
    int in_unit, out_unit, taps_max, pitch, first_min, first_span, tile, span;      // first_span = first_max - first_min
};

// LDS, in 4-byte words: the weight rows [out_unit][pitch], first[i] - first_min as int [out_unit], the staged samples [span]
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(RsParams p, const float* __restrict__ tables, const int16_t* __restrict__ pcm,
                                                              const long* __restrict__ offsets, const int* __restrict__ samples,
                                                              const long* __restrict__ out_offsets, int16_t* __restrict__ out_pcm,
                                                              float* __restrict__ out_f32, int* __restrict__ out_samples, int* __restrict__ clipped) {
    XV_EW_PRIORITY();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int count[RS_THREADS];
    const int tid = threadIdx.x, u = blockIdx.y;
    float* wl = lds;
    int* fl = (int*)(lds + (size_t)p.out_unit * p.pitch);
    float* xs = (float*)(fl + p.out_unit);
    const long n = samples[u] > 0 ? samples[u] : 0;
    const long n_out = (n * p.out_unit + p.in_unit - 1) / p.in_unit;
    if (blockIdx.x == 0 && tid == 0) out_samples[u] = (int)n_out;
    const long tiles = (n_out + p.tile - 1) / p.tile;
    if ((long)blockIdx.x >= tiles) return;      // uniform
    // a table that is not xv_resample_tables' own must not send a read outside LDS: first is clamped to the range the span was sized for
    for (int e = tid; e < p.out_unit; e += RS_THREADS) fl[e] = min(max((int)tables[e] - p.first_min, 0), p.first_span);
    for (int e = tid; e < p.out_unit * p.taps_max; e += RS_THREADS) {
        const int i = e / p.taps_max, j = e - i * p.taps_max;
        wl[i * p.pitch + j] = tables[2 * p.out_unit + e];
    }
    const int16_t* x = pcm + offsets[u];
    const long out_off = out_offsets[u];
    for (long ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        __syncthreads();      // the table is in place; the tile before is done with xs and count
        const long o0 = ti * p.tile, q0 = o0 / p.out_unit;
        const int i0 = (int)(o0 - q0 * p.out_unit);
        const long base = (long)p.first_min + q0 * p.in_unit;      // xs[k] = x[base + k]
        for (int k = tid; k < p.span; k += RS_THREADS) {
            const long g = base + k;
            xs[k] = (g >= 0 && g < n) ? (float)x[g] : 0.f;
        }
        __syncthreads();
        const float* wr[RS_R];
        const float* xr[RS_R];
        float acc[RS_R];
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const int t = tid + r * RS_THREADS;
            const unsigned ii = (unsigned)(i0 + (t < p.tile ? t : 0));      // a lane beyond the tile reads where output 0 does
            const unsigned qr = ii / (unsigned)p.out_unit, ph = ii - qr * (unsigned)p.out_unit;
            wr[r] = wl + ph * p.pitch;
            xr[r] = xs + fl[ph] + qr * p.in_unit;
            acc[r] = 0.f;
        }
#pragma unroll 1
        for (int j = 0; j < p.taps_max; ++j) {
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(wr[r][j], xr[r][j], acc[r]);
        }
        int changed = 0;
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const int t = tid + r * RS_THREADS;
            if (t < p.tile && o0 + t < n_out) {
                const float v = rintf(acc[r]), c = fminf(fmaxf(v, -32768.f), 32767.f);
                changed += c != v;
                out_pcm[out_off + o0 + t] = (int16_t)c;
                if (out_f32) out_f32[out_off + o0 + t] = acc[r];
            }
        }
        count[tid] = changed;
        __syncthreads();
        for (int o = RS_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) count[tid] += count[tid + o];
            __syncthreads();
        }
        if (tid == 0 && count[0]) atomicAdd(clipped + u, count[0]);      // an integer count: its value does not depend on the order
    }
}

extern "C" int xv_resample(void* stream, const xv_resample_config* cfg, const float* tables_dev, const int16_t* pcm, const int64_t* offsets,
                           const int32_t* samples, int b, const int64_t* out_offsets, int16_t* out_pcm, float* out_f32, int32_t* out_samples,
                           int32_t* clipped) {
    RsDims d;
    if (int rc = rs_dims(cfg, &d)) return rc;
    XV_REQUIRE(tables_dev && pcm && offsets && samples && out_offsets && out_pcm && out_samples && clipped && b > 0, "resample: bad arguments");
    XV_REQUIRE(b <= 65535, "resample: at most 65535 utterances a call (got %d)", b);
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    RsParams p;
    p.in_unit = d.in_unit; p.out_unit = d.out_unit; p.taps_max = d.taps_max; p.pitch = d.pitch;
    p.first_min = d.first_min; p.first_span = d.first_max - d.first_min; p.tile = d.tile; p.span = d.span;
    hipStream_t s = (hipStream_t)stream;
    XV_CHECK_HIP(hipMemsetAsync(clipped, 0, (size_t)b * sizeof(int32_t), s));
    if (d.lds_bytes > 64 * 1024)
        XV_CHECK_HIP(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)d.lds_bytes));
    // tiles walked per utterance: enough workgroups for the device when the batch is small, fewer copies of the table when it is large
    int gx = 4096 / b;
    gx = gx < 8 ? 8 : gx > 1024 ? 1024 : gx;
    hipLaunchKernelGGL(resample_kernel, dim3(gx, b), dim3(RS_THREADS), d.lds_bytes, s, p, tables_dev, pcm, (const long*)offsets, (const int*)samples,
                       (const long*)out_offsets, out_pcm, out_f32, (int*)out_samples, (int*)clipped);
    XV_LAUNCH_CHECK();
    return 0;
}
