// Diarization error counts on the device (xv_diar_confusion; include/xvector_hip.h states the arithmetic, tests/diar_eval_ref.py restates
// it): what md-eval counts per frame - scored speaker time, missed and falsely alarmed speaker time, and the time every reference speaker
// shares with every hypothesis cluster - for b recordings at many cuts (label sets) in one launch.  The reference of a recording (speaker
// bit mask, scored flag and owning window per 10 ms frame) is uploaded once and read by every cut.  md-eval is restated from its
// definition; nothing is compared with a run of it.  gfx950 only.
//
// One workgroup per (recording, cut), no hand-over between workgroups.  Every output is an integer: the totals are int64 sums of small
// non-negative integers, the overlap counts are int32 adds into a histogram in LDS (32 speakers x 256 clusters, 32 KB).  Integer adds
// commute, so the result is exact and independent of the order in which lanes, waves or atomics arrive: the same bytes every time.
//
// A frame costs 9 bytes of loads (mask, flag, window), coalesced over the lanes, and one gather of its window's label, which the 75 to
// 150 consecutive frames of a window share; a scored frame with speech adds one LDS atomic per reference speaker of the frame.
#include "xv_common.h"
#include "xv_ew.h"

#define DE_THREADS 256
#define DE_WAVES (DE_THREADS / XV_WAVE)
#define DE_MAX_SPEAKERS 32
#define DE_MAX_CLUSTERS 256

struct DiarEvalArgs {
    const uint32_t* ref_mask; const uint8_t* scored; const int32_t* frame_window;
    const int64_t* frame_offsets; const int64_t* win_offsets; const int32_t* speakers;
    int b; long total_frames, total_n;
    const int32_t* labels; const int32_t* clusters; const int64_t* out_offsets; long overlap_ints;
    int64_t* totals; int32_t* overlap; int32_t* status;
};

__global__ __launch_bounds__(DE_THREADS) void diar_confusion_kernel(DiarEvalArgs g) {
    XV_EW_PRIORITY();
    __shared__ int hist[DE_MAX_SPEAKERS * DE_MAX_CLUSTERS];
    __shared__ long red[3][DE_WAVES];
    __shared__ int any_bad;
    const int r = blockIdx.x, cut = blockIdx.y, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), w = tid / XV_WAVE;
    const long block = (long)cut * g.b + r;
    const long f0 = g.frame_offsets[r], f1 = g.frame_offsets[r + 1], w0 = g.win_offsets[r], w1 = g.win_offsets[r + 1];
    const int S = g.speakers[r], K = g.clusters[block];
    const long o0 = g.out_offsets[block];
    int64_t* totals = g.totals + 3 * block;
    // (uniform) a block whose entries would take the kernel outside the buffers of the call is skipped; so is a cut with more clusters than
    // the histogram holds, which says so
    const bool inside = f0 >= 0 && f0 <= f1 && f1 <= g.total_frames && w0 >= 0 && w0 < w1 && w1 <= g.total_n && S >= 1 && S <= DE_MAX_SPEAKERS && K >= 1;
    const bool counted = inside && K <= DE_MAX_CLUSTERS;
    if (!counted || o0 < 0 || o0 + (long)S * K > g.overlap_ints) {
        if (tid == 0) {
            g.status[block] = inside && K > DE_MAX_CLUSTERS ? 1 : -1;
            totals[0] = totals[1] = totals[2] = 0;
        }
        return;
    }
    for (int i = tid; i < S * K; i += DE_THREADS) hist[i] = 0;
    if (tid == 0) any_bad = 0;
    __syncthreads();
    const int32_t* __restrict__ lab = g.labels + (long)cut * g.total_n + w0;
    const int windows = (int)min(w1 - w0, (long)INT32_MAX);
    const uint32_t keep = S == 32 ? 0xffffffffu : (1u << S) - 1u;      // (bits at and above S are no speakers of this recording)
    long speech = 0, miss = 0, fa = 0;
    bool bad = false;
    for (long f = f0 + tid; f < f1; f += DE_THREADS) {
        const uint32_t ref = g.ref_mask[f] & keep;
        const int win = g.frame_window[f];
        if (!g.scored[f]) continue;
        int h = -1;
        if (win >= 0) {
            if (win < windows) h = lab[win];
            if (h < 0 || h >= K) { bad = true; continue; }      // a window or a label outside the call: the block is refused below
        }
        const int pc = __popc(ref), has = h >= 0 ? 1 : 0;
        speech += pc;
        miss += max(0, pc - has);
        fa += max(0, has - pc);
        if (has)
            for (uint32_t m = ref; m; m &= m - 1) atomicAdd(&hist[(__ffs(m) - 1) * K + h], 1);
    }
    if (bad) any_bad = 1;      // (every writer stores the same value)
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) {
        speech += __shfl_xor(speech, off);
        miss += __shfl_xor(miss, off);
        fa += __shfl_xor(fa, off);
    }
    if (lane == 0) { red[0][w] = speech; red[1][w] = miss; red[2][w] = fa; }
    __syncthreads();
    if (any_bad) {      // (uniform)
        if (tid == 0) {
            g.status[block] = -1;
            totals[0] = totals[1] = totals[2] = 0;
        }
        return;
    }
    if (tid < 3) {
        long sum = 0;
#pragma unroll
        for (int i = 0; i < DE_WAVES; ++i) sum += red[tid][i];
        totals[tid] = sum;
    }
    if (tid == 0) g.status[block] = 0;
    for (int i = tid; i < S * K; i += DE_THREADS) g.overlap[o0 + i] = hist[i];
}

extern "C" int xv_diar_confusion(void* stream, const uint32_t* ref_mask, const uint8_t* scored, const int32_t* frame_window,
                                 const int64_t* frame_offsets, const int64_t* win_offsets, const int32_t* speakers, int b, int64_t total_frames,
                                 int64_t total_n, const int32_t* labels, const int32_t* clusters, const int64_t* out_offsets, int cuts,
                                 int64_t overlap_ints, int64_t* totals, int32_t* overlap, int32_t* status) {
    XV_REQUIRE(b > 0, "diar_confusion: no recording in the call (b=%d)", b);
    XV_REQUIRE(cuts > 0 && cuts <= 65535, "diar_confusion: 1 .. 65535 cuts in a call (cuts=%d)", cuts);
    XV_REQUIRE(total_frames >= 0 && total_n >= b && overlap_ints >= 0, "diar_confusion: total_frames / total_n / overlap_ints do not fit %d recordings", b);
    XV_REQUIRE(frame_offsets && win_offsets && speakers && labels && clusters && out_offsets && totals && status, "diar_confusion: bad arguments");
    XV_REQUIRE(total_frames == 0 || (ref_mask && scored && frame_window), "diar_confusion: ref_mask, scored and frame_window are needed (there are frames)");
    XV_REQUIRE(overlap_ints == 0 || overlap, "diar_confusion: overlap is needed (overlap_ints=%lld)", (long long)overlap_ints);
    DiarEvalArgs g;
    g.ref_mask = ref_mask; g.scored = scored; g.frame_window = frame_window;
    g.frame_offsets = frame_offsets; g.win_offsets = win_offsets; g.speakers = speakers;
    g.b = b; g.total_frames = (long)total_frames; g.total_n = (long)total_n;
    g.labels = labels; g.clusters = clusters; g.out_offsets = out_offsets; g.overlap_ints = (long)overlap_ints;
    g.totals = totals; g.overlap = overlap; g.status = status;
    hipLaunchKernelGGL(diar_confusion_kernel, dim3(b, cuts), dim3(DE_THREADS), 0, (hipStream_t)stream, g);
    XV_LAUNCH_CHECK();
    return 0;
}
