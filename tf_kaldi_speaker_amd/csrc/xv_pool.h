// Engine forms of the pooling and attention entry points (xv_pool.hip, xv_attention.hip).
#pragma once
#include "xv_common.h"

// Statistics pooling fused with the last frame layer's BatchNorm, engine form (xv_pool.hip): the forward also writes
// wpos [b][c] = the share of each chunk's frame weights on frames with an active ReLU; given that, the BatchNorm backward gets its
// two reductions in closed form from the pooled statistics instead of a pass over z (plain ReLU / no activation); amax [b][c] = each
// chunk's largest activation, which bounds |d a| for the split-precision dz scale (XvBnUpstream.wpos / .pamax, unit frame weights)
// frames (optional, device [b]) / shrink: chunk i pools only its first frames[i] - shrink rows (batched extraction: utterances of different
// lengths padded to t rows; shrink = the frames the frame layers consumed)
int xv_stat_pool_forward_bn_ex(hipStream_t s, const float* z, int b, int t, int c, const float* scale, const float* shift, int relu,
                               const float* weights, float* out, float* wpos, float* amax, const int32_t* frames = nullptr, int shrink = 0,
                               int ldz = 0 /* floats per row of z; 0 = c */);
// xv_vlad_pool_forward on a hipStream_t (xv_vlad.hip)
int xv_vlad_pool_forward_ex(hipStream_t s, const float* x, const float* a, const float* centers, int b, int t, int c, int k, int kg,
                            const int32_t* frames, int shrink, float* r, float* n);
// softmax over the first frames[i] - shrink scores of chunk i (weights beyond are 0); frames == nullptr: all t (xv_attention.hip)
int xv_softmax_segments_ex(hipStream_t s, const float* score, int b, int t, float* weights, const int32_t* frames, int shrink);
