// Feature front end of extraction: Kaldi's sliding-window cepstral mean normalisation and voiced-frame selection on a padded batch of raw
// utterances - what `apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=W | select-voiced-frames` do in the pipe in front of
// the reference's extract.py (egs/voxceleb/v1/nnet/run_extract_embeddings.sh:47) - applied right behind xv_cm_decode_ragged.  Two
// launches: a scan of every piece's voicing mask into the raw indices of the rows it keeps, then the window means (double) and the
// gather.  No atomics and no cross-workgroup hand-over: a result depends on the shape of the call only, so it is the same bits every
// time.  gfx950 only.
#include "xv_common.h"
#include "xv_ew.h"

#define FE_MAX_D 128          // the decoder's limit (CMD_MAX_D, xv_prep.hip): these kernels run on what it wrote
#define FE_SCAN_THREADS 256
#define FE_ROWS 16            // consecutive output rows one thread group walks with a running window sum
#define FE_MAX_GROUPS 16      // thread groups (of d lanes: one per column) in a workgroup of 256

// frames of piece i the kernels may touch, its first kept row and how many it may write
__device__ __forceinline__ int fe_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sel[i][j] = raw index of the (first[i] + j)-th voiced frame of piece i for j < rows_out[i] = min(count[i], voiced - first[i]).
// One workgroup per piece walks the mask 256 frames at a time: a ballot gives every voiced lane its rank inside the wave, four wave
// totals (LDS) its rank inside the step, a running total its rank in the utterance.
__global__ __launch_bounds__(FE_SCAN_THREADS) void frontend_scan_kernel(const uint8_t* __restrict__ masks, long mask_bytes, const long* __restrict__ moffs,
                                                                        const int* __restrict__ rows_in, int t_in, const int* __restrict__ first,
                                                                        const int* __restrict__ count, int t_out, int* __restrict__ sel,
                                                                        int* __restrict__ rows_out) {
    XV_EW_PRIORITY();
    __shared__ int wtot[FE_SCAN_THREADS / XV_WAVE];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), wave = tid / XV_WAVE;
    const int n = fe_clamp(rows_in[i], 0, t_in);
    const int f0 = first ? max(first[i], 0) : 0;
    const int cnt = fe_clamp(count ? count[i] : t_out, 0, t_out);
    const long mo = moffs[i];
    int* s = sel + (long)i * t_out;
    int seen = 0;      // voiced frames in front of this step (the same in every thread)
    for (int t0 = 0; t0 < n; t0 += FE_SCAN_THREADS) {
        const int t = t0 + tid;
        // a mask byte outside the buffer the caller handed over counts as unvoiced (the offsets live on the device: nothing on the host saw them)
        const bool v = t < n && mo >= 0 && mo + t < mask_bytes && masks[mo + t] != 0;
        const unsigned long long bal = __ballot(v);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int before = seen, step = 0;
#pragma unroll
        for (int k = 0; k < FE_SCAN_THREADS / XV_WAVE; ++k) {
            if (k < wave) before += wtot[k];
            step += wtot[k];
        }
        const int pos = before + __popcll(bal & ((1ull << lane) - 1ull)) - f0;
        if (v && pos >= 0 && pos < cnt) s[pos] = t;
        seen += step;
        __syncthreads();
        if (seen - f0 >= cnt) break;      // uniform: everything this piece keeps is written
    }
    if (tid == 0) rows_out[i] = fe_clamp(seen - f0, 0, cnt);
}

// out[i][j][:] = x[i][t][:] - mean(x[i][s:e][:]) for t = sel[i][j] (no mask: first[i] + j), [s, e) the window of SlidingWindowCmn with
// center = true around t (feature-functions.cc), rows j >= rows_out[i] zero.  A workgroup = `groups` thread groups of d lanes (one lane
// per column); a group walks FE_ROWS consecutive output rows: the window of its first row summed outright, the following ones by
// dropping the rows that left and adding the rows that entered (t only grows, so both window ends only move forward) - in double, as
// Kaldi's own running sums are, so the order of the additions is far below the single fp32 rounding of the result.
template <bool MASKED>
__global__ __launch_bounds__(256) void frontend_cmn_select_kernel(const float* __restrict__ x, const int* __restrict__ rows_in, int t_in, int d, int w,
                                                                  const int* __restrict__ sel, const int* __restrict__ first,
                                                                  const int* __restrict__ count, int t_out, float* __restrict__ out,
                                                                  int* __restrict__ rows_out, int groups) {
    XV_EW_PRIORITY();
    const int i = blockIdx.y, tid = threadIdx.x;
    const int g = tid / d, c = tid - g * d;
    const int n = fe_clamp(rows_in[i], 0, t_in);
    const int f0 = first ? max(first[i], 0) : 0;
    int nrow;
    if (MASKED) nrow = rows_out[i];      // written by the scan launch in front of this one
    else {
        nrow = fe_clamp(n - f0, 0, fe_clamp(count ? count[i] : t_out, 0, t_out));
        if (blockIdx.x == 0 && tid == 0) rows_out[i] = nrow;
    }
    if (g >= groups) return;
    const float* xi = x + (long)i * t_in * d + c;
    float* oi = out + (long)i * t_out * d + c;
    const int* si = sel + (long)i * t_out;
    const int j0 = (blockIdx.x * groups + g) * FE_ROWS;
    const int j1 = min(j0 + FE_ROWS, t_out);
    double sum = 0.0;
    int ps = 0, pe = 0;      // the window `sum` holds: x[ps .. pe)
    for (int j = j0; j < j1; ++j) {
        if (j >= nrow) { oi[(long)j * d] = 0.f; continue; }
        const int t = MASKED ? si[j] : f0 + j;
        const float v = xi[(long)t * d];
        if (w <= 0) { oi[(long)j * d] = v; continue; }
        int s = t - w / 2, e = s + w;
        if (s < 0) { e -= s; s = 0; }
        if (e > n) { s -= e - n; e = n; s = max(s, 0); }
        if (s >= pe) {      // first row of the group, or the voiced rows jumped past the whole window
            sum = 0.0;
            ps = pe = s;
        }
#pragma unroll 4
        for (int r = ps; r < s; ++r) sum -= (double)xi[(long)r * d];
#pragma unroll 4
        for (int r = pe; r < e; ++r) sum += (double)xi[(long)r * d];
        ps = s; pe = e;
        oi[(long)j * d] = (float)((double)v - sum / (double)(e - s));
    }
}

extern "C" int xv_frontend(void* stream, const float* x, const int32_t* rows_in, int b, int t_in, int d, int cmn_window, const uint8_t* masks,
                           size_t mask_bytes, const int64_t* mask_offsets, const int32_t* first, const int32_t* count, int t_out, float* out,
                           int32_t* rows_out, void* ws, size_t ws_bytes) {
    XV_REQUIRE(x && rows_in && out && rows_out && x != out && b > 0 && t_in > 0 && t_out > 0 && d > 0, "frontend: bad arguments");
    XV_REQUIRE(d <= FE_MAX_D, "frontend: at most %d feature dimensions (got %d)", FE_MAX_D, d);
    XV_REQUIRE(cmn_window >= 0 && cmn_window <= (1 << 30), "frontend: the CMN window must lie in 0 .. 2^30 (got %d)", cmn_window);
    XV_REQUIRE(b <= 65535, "frontend: at most 65535 pieces a call (got %d)", b);
    XV_REQUIRE(!masks || mask_offsets, "frontend: masks without their offsets");
    static_assert(sizeof(long) == sizeof(int64_t), "offsets are passed as long");
    hipStream_t s = (hipStream_t)stream;
    int* sel = nullptr;
    if (masks) {
        const size_t need = (size_t)b * t_out * sizeof(int);
        XV_REQUIRE(ws && ws_bytes >= need, "frontend: workspace of %zu bytes, %zu needed (b * t_out * 4)", ws_bytes, need);
        sel = (int*)ws;
        hipLaunchKernelGGL(frontend_scan_kernel, dim3(b), dim3(FE_SCAN_THREADS), 0, s, masks, (long)mask_bytes, (const long*)mask_offsets,
                           (const int*)rows_in, t_in, (const int*)first, (const int*)count, t_out, sel, (int*)rows_out);
        XV_LAUNCH_CHECK();
    }
    const int groups = min(256 / d, FE_MAX_GROUPS);
    dim3 grid(xv_cdiv(t_out, (long)groups * FE_ROWS), b);
    if (masks)
        hipLaunchKernelGGL(frontend_cmn_select_kernel<true>, grid, dim3(256), 0, s, x, (const int*)rows_in, t_in, d, cmn_window, (const int*)sel,
                           (const int*)first, (const int*)count, t_out, out, (int*)rows_out, groups);
    else
        hipLaunchKernelGGL(frontend_cmn_select_kernel<false>, grid, dim3(256), 0, s, x, (const int*)rows_in, t_in, d, cmn_window, (const int*)sel,
                           (const int*)first, (const int*)count, t_out, out, (int*)rows_out, groups);
    XV_LAUNCH_CHECK();
    return 0;
}
