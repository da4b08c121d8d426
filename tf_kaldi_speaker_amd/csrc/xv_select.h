// The exact top-k selection over one row of scores, and its mean / deviation: the kernel the cohort statistics of cosine scoring
// (xv_score.hip: an element is a slab float) and of PLDA scoring (xv_backend_cohort.hip: an element is a slab float plus a column term plus
// a row term) share.  How an element is loaded is the template parameter; everything else is stated once.  It is a kernel template, not a
// function the two kernels inline: the body then sits in the kernel itself as it did before it was shared, and sc_select_kernel<ScSlabRow>
// is instruction for instruction the score_select_kernel it replaces (profiles/plda_cohort_registers.txt).  gfx950 only.
#pragma once
#include "xv_common.h"
#include "xv_ew.h"
#include "xv_radix_key.h"   // sc_key / sc_unkey: the unsigned key whose order is the float's

#define SC_SEL_THREADS 256
#define SC_TILE_ROWS 128          // the score slab holds a whole number of GEMM row tiles

// floats per slab row: the cohort size on the 16-byte grid
static inline size_t sc_slab_pitch(int n_cohort) { return xv_align((size_t)(n_cohort > 0 ? n_cohort : 1), 4); }

// a double summed over the workgroup in a fixed order: butterfly inside each wave, the four wave totals added first to last
__device__ __forceinline__ double sc_block_sum(double v, double* wtot, int tid) {
    v = wave_sum(v);
    __syncthreads();      // (wtot may still be read from the call before)
    if ((tid & 63) == 0) wtot[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SC_SEL_THREADS / XV_WAVE; ++w) s += wtot[w];
    return s;
}

// A Row is built once per workgroup from (the workgroup's slab row, the slab's pitch, the launch's extra arguments...).
// The plain element: row[i].  load4(q) = the elements 4q .. 4q + 3 (the row starts on a 16-byte boundary), load1(i) = element i.
struct ScSlabRow {
    const float* row;
    __device__ __forceinline__ ScSlabRow(const float* r, long) : row(r) {}
    __device__ __forceinline__ f32x4 load4(int q) const { return *(const f32x4*)(row + 4 * q); }
    __device__ __forceinline__ float load1(int i) const { return row[i]; }
};

// stats[r] = (mean, sqrt(max(var, 1e-12))) of the k largest of the n elements of row r = blockIdx.x (k <= n), an element being what
// Row(slab + r * lds, lds, extra...) loads.  One workgroup of SC_SEL_THREADS per row; every slab row starts on a 16-byte boundary (the slab
// is 16-byte aligned and lds a multiple of 4).
// Radix select of the k-th largest key, most significant byte first: each pass counts, among the elements that share the bytes already
// fixed, the next byte's 256 values in LDS; wave 0 walks the counts from the top until `want` more elements are covered, which fixes the
// byte and leaves `want` = the rank inside that bucket.  After four passes the key is the k-th largest score exactly and `want` is how
// many copies of it the top k holds (k - want elements lie strictly above).  The sums take the elements strictly above plus `want` copies
// of the threshold, so a cut through a run of equal scores is well defined; they are accumulated in double (a thread's elements in index
// order, then sc_block_sum), the variance around the mean in a second pass.  The row is streamed six times; nothing of it is kept in LDS,
// so n is not bounded here.  The select is exact only if all six passes see the same bits of an element: Row's two loads must be a pure
// function of the index.
template <class Row, class... Extra>
__global__ __launch_bounds__(SC_SEL_THREADS) void sc_select_kernel(const float* __restrict__ slab, long lds, int n, int k, float* __restrict__ stats,
                                                                    Extra... extra) {
    XV_EW_PRIORITY();
    __shared__ int hist[256];
    __shared__ unsigned sh_prefix;
    __shared__ int sh_want;
    __shared__ double wtot[SC_SEL_THREADS / XV_WAVE];
    const int tid = threadIdx.x;
    const Row row(slab + (long)blockIdx.x * lds, lds, extra...);
    const int n4 = n / 4;
    unsigned prefix = 0, mask = 0;
    int want = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int q = tid; q < n4; q += SC_SEL_THREADS) {
            const f32x4 v = row.load4(q);
            const unsigned k0 = sc_key(v.x), k1 = sc_key(v.y), k2 = sc_key(v.z), k3 = sc_key(v.w);
            if ((k0 & mask) == prefix) atomicAdd(&hist[(k0 >> shift) & 255u], 1);
            if ((k1 & mask) == prefix) atomicAdd(&hist[(k1 >> shift) & 255u], 1);
            if ((k2 & mask) == prefix) atomicAdd(&hist[(k2 >> shift) & 255u], 1);
            if ((k3 & mask) == prefix) atomicAdd(&hist[(k3 >> shift) & 255u], 1);
        }
        if (tid < n - 4 * n4) {
            const unsigned kk = sc_key(row.load1(4 * n4 + tid));
            if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid < XV_WAVE) {      // lane l owns the buckets 255 - 4l ... 252 - 4l, walked downwards
            int c[4], own = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = hist[255 - 4 * tid - j]; own += c[j]; }
            int incl = own;
#pragma unroll
            for (int o = 1; o < XV_WAVE; o <<= 1) {
                const int up = __shfl_up(incl, o);
                if (tid >= o) incl += up;
            }
            int above = incl - own;      // elements in the buckets of the lanes in front
            if (above < want && want <= incl) {      // exactly one lane: the buckets hold at least `want` elements together
                int digit = 255 - 4 * tid - 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (want <= above + c[j]) { digit = 255 - 4 * tid - j; break; }
                    above += c[j];
                }
                sh_prefix = prefix | ((unsigned)digit << shift);
                sh_want = want - above;
            }
        }
        __syncthreads();
        prefix = sh_prefix;
        want = sh_want;
        mask |= 255u << shift;
    }
    const float thr = sc_unkey(prefix);
    const double dthr = (double)thr;
    double acc = 0.0;
    for (int q = tid; q < n4; q += SC_SEL_THREADS) {
        const f32x4 v = row.load4(q);
        if (sc_key(v.x) > prefix) acc += (double)v.x;
        if (sc_key(v.y) > prefix) acc += (double)v.y;
        if (sc_key(v.z) > prefix) acc += (double)v.z;
        if (sc_key(v.w) > prefix) acc += (double)v.w;
    }
    if (tid < n - 4 * n4) {
        const float v = row.load1(4 * n4 + tid);
        if (sc_key(v) > prefix) acc += (double)v;
    }
    const double mean = (sc_block_sum(acc, wtot, tid) + (double)want * dthr) / (double)k;
    acc = 0.0;
    for (int q = tid; q < n4; q += SC_SEL_THREADS) {
        const f32x4 v = row.load4(q);
        if (sc_key(v.x) > prefix) acc += ((double)v.x - mean) * ((double)v.x - mean);
        if (sc_key(v.y) > prefix) acc += ((double)v.y - mean) * ((double)v.y - mean);
        if (sc_key(v.z) > prefix) acc += ((double)v.z - mean) * ((double)v.z - mean);
        if (sc_key(v.w) > prefix) acc += ((double)v.w - mean) * ((double)v.w - mean);
    }
    if (tid < n - 4 * n4) {
        const float v = row.load1(4 * n4 + tid);
        if (sc_key(v) > prefix) acc += ((double)v - mean) * ((double)v - mean);
    }
    const double var = (sc_block_sum(acc, wtot, tid) + (double)want * (dthr - mean) * (dthr - mean)) / (double)k;
    if (tid == 0) {
        stats[2 * (long)blockIdx.x] = (float)mean;
        stats[2 * (long)blockIdx.x + 1] = (float)sqrt(fmax(var, 1e-12));
    }
}
