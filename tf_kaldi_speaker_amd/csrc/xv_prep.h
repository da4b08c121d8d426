#pragma once
#include "xv_common.h"

// All kernel-layout weight copies of one optimiser step in two launches (xv_prep.hip): the per-layer
// prep / amax / split launches (~25 of 5 us each) were 5 % of a step.
enum { XV_PREP_T32 = 0,     // wt[o][j*c_pad + c] = w[(j*C + c)*O + o]                (fp32, forward layout)
       XV_PREP_F32 = 1,     // wf[c][(k-1-j)*o_ld + o] = w[(j*C + c)*O + o]           (fp32, tap-flipped data-gradient layout)
       XV_PREP_T16 = 2,     // as T32, written as two fp16 planes scaled by pow2(*amax)
       XV_PREP_F16 = 3 };   // as F32, planes
struct XvPrepJob {
    int type, k, C, O, c_pad, o_ld;
    int tiles_x, tile0;              // 32x32 tiles per row of tiles, first global tile index
    const float* w;
    void* dst;
    long plane;                      // plane stride in elements (16-bit types)
    const unsigned* amax;
};
#define XV_PREP_PAD 8            // not a weight: rows [O][C] of w copied into [O][c_pad] with zero pad columns (the features of a step, riding on the first layer's launch)
#define XV_PREP_MAX_JOBS 32      // two layouts x (XV_MAX_FRAME_LAYERS + 2 segment + 2 attention-key layers)
struct XvPrepJobs { int n, total_tiles; XvPrepJob j[XV_PREP_MAX_JOBS]; };
#define XV_AMAX_MAX_JOBS 16
struct XvAmaxJobs { int n; const float* x[XV_AMAX_MAX_JOBS]; size_t count[XV_AMAX_MAX_JOBS]; unsigned* out[XV_AMAX_MAX_JOBS]; };
int xv_prep_add(XvPrepJobs& J, int type, const float* w, int k, int C, int O, int c_pad, int o_ld, void* dst, long plane, const unsigned* amax);
int xv_launch_weight_prep(hipStream_t s, const XvPrepJobs& J);
int xv_launch_amax_multi(hipStream_t s, const XvAmaxJobs& J);
