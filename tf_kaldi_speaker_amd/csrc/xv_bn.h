// Engine-internal BatchNorm forms (xv_bn.hip, xv_bn_bwd.hip).
#pragma once
#include "xv_common.h"

// Segment-level BatchNorm (rows = chunks per batch, a few hundred at most) in ONE launch each way: statistics, moving
// averages, scale/shift and the activation (forward); both reductions and dz (backward).  The three-kernel forms are
// built for 25 k-row tensors; on 128 rows their launches and gaps were what the layer cost.  (xv_bn.hip)
#define XV_BN_SMALL_MAX_ROWS 4096
int xv_bn_small_forward(hipStream_t s, const float* z, int rows, int n, const float* gamma, const float* beta, float eps, float momentum,
                        int unbiased_moving, float* moving_mean, float* moving_var, float* mean, float* invstd, float* scale, float* shift,
                        int relu, float* a);
int xv_bn_small_backward(hipStream_t s, const float* da, const float* z, int rows, int n, const float* gamma, const float* mean,
                         const float* invstd, const float* scale, const float* shift, int relu, float* dz, float* dgamma, float* dbeta,
                         float* dbias);

// BatchNorm (+ activation) backward of a frame-level layer, the engine-internal forms behind the xv_bn_relu_backward* family (xv_bn_bwd.hip).
// XvBnUpstream says where the upstream gradient comes from: the tensor `da`, or - pool_out != null - the (weighted) statistics-pooling
// backward of (pool_out, dpool) over chunks of pool_t frames, evaluated on the fly.  wpos / pamax [b][n] (optional, from
// xv_stat_pool_forward_bn_ex): with wpos and a plain ReLU the two reductions have a closed form and the pass over z is skipped; pamax
// bounds |d a| for the split-precision dz scale (unit frame weights).  ext_part [ext_chunks][3][n]: the reductions of `da` already done by
// a GEMM epilogue (xv_epilogue.h XvBwdStats).
struct XvBnUpstream { const float* da; const float* pool_out; const float* dpool; int pool_t; const float* weights; const float* wpos;
                      const float* pamax; const float* ext_part; int ext_chunks; };
// dz in fp32; ldz: floats per row of z and dz, 0 = n; a pitch needs wpos (the closed form) and a plain ReLU
int xv_bn_backward_f32(hipStream_t s, const XvBnUpstream& up, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                       const float* invstd, const float* scale, const float* shift, int relu, int pad, float* dz_pad, int ldz, float* dgamma,
                       float* dbeta, float* dbias, void* ws, size_t ws_bytes);
// dz as fp16 planes; zero_amax = false: *dz_amax was zeroed by the caller (one memset per backward pass instead of one per layer)
int xv_bn_backward_split(hipStream_t s, const XvBnUpstream& up, const float* z, int segs, int t, int n, const float* gamma, const float* mean,
                         const float* invstd, const float* scale, const float* shift, const float* zmin, const float* zmax, int relu, int pad,
                         void* dz_planes, int ldp, size_t plane_stride, uint32_t* dz_amax, bool zero_amax, float* dgamma, float* dbeta,
                         float* dbias, void* ws, size_t ws_bytes);

// a = act(z) (da == nullptr) or dz = da * act'(z) + d alpha (segment-level tensors, rows <= XV_BN_SMALL_MAX_ROWS): a layer with the
// activation but no BatchNorm in front (tdnn7 with last_layer_no_bn); the activation is the act context's (xv_ew.h)
int xv_act_small(hipStream_t s, const float* da, const float* z, int rows, int n, float* out);
