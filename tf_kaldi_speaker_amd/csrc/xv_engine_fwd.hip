// Engine, forward: the kernel-layout weight copies of a step (prep_layers, ensure_weights and the two waits for their side-stream
// halves), the forward pass - frame layers, pooling (xv_engine_pool.hip), segment layers, output - in both precisions, the preamble of
// the loss head's forward (xv_engine_head.hip), and the regularisation loss.  Everything here is enqueued on the caller's stream except the overlapped weight copies.
#include <algorithm>

#include "xv_engine.h"

// Kernel-layout (and, in split precision, fp16-plane) copies of the weights, rebuilt after every update: one memset + one
// multi-tensor amax + one multi-job layout kernel (+ the loss head's two) instead of ~28 launches.
// With `overlap` (the training forward pass) only the FIRST layer's copies are made on `s`; the other layers' and the loss
// head's go to the side stream behind an event on `s` and are waited for where they are first used (xve_wait_prep before the
// second layer, xve_wait_lossprep before the logits) - they then run under the feature split / first GEMM instead of in front
// of them (58 us of a 5.8 ms fp32 step, 112 us of a 2.7 ms f16x3 step were spent there with the chip otherwise idle).
int xve_wait_prep(xv_engine* e, hipStream_t s) {
    if (e->prep_pending) { XV_CHECK_HIP(hipStreamWaitEvent(s, e->ev_prep, 0)); e->prep_pending = false; }
    return 0;
}
int xve_wait_lossprep(xv_engine* e, hipStream_t s) {
    if (e->lossprep_pending) { XV_CHECK_HIP(hipStreamWaitEvent(s, e->ev_lossprep, 0)); e->lossprep_pending = false; }
    return 0;
}

namespace {

int prep_layers(xv_engine* e, hipStream_t s, int first, int last) {
    XvPrepJobs J = {};
    XvAmaxJobs A = {};
    for (int i = first; i < last; ++i) {
        XvAffine& a = e->L[i];
        const float* w = vptr(e, a.v_kernel);
        if (e->f16 && is_frame(e, i)) {
            // fp16 planes scaled by the tensor's own max |w|; the forward and dgrad layouts hold the same values, so one
            // max per layer, taken on the variable itself
            const unsigned* am = e->amax + AMAX_WT + a.wslot;
            XV_REQUIRE(A.n < XV_AMAX_MAX_JOBS, "ensure_weights: too many weight tensors for one amax launch");
            A.x[A.n] = w; A.count[A.n] = (size_t)a.k * a.c_in * a.c_out; A.out[A.n] = e->amax + AMAX_WT + a.wslot; A.n++;
            int rc = xv_prep_add(J, XV_PREP_T16, w, a.k, a.c_in, a.c_out, a.c_pad, a.o_ld, a.wth, (long)a.wth_stride, am);
            if (rc) return rc;
            if (i > 0) {
                rc = xv_prep_add(J, XV_PREP_F16, w, a.k, a.c_in, a.c_out, a.c_pad, a.o_ld, a.wfh, (long)a.wfh_stride, am);
                if (rc) return rc;
            }
        } else {
            int rc = xv_prep_add(J, XV_PREP_T32, w, a.k, a.c_in, a.c_out, a.c_pad, a.c_out, a.wt, 0, nullptr);
            if (rc) return rc;
            if (a.k > 1 && i > 0) {
                rc = xv_prep_add(J, XV_PREP_F32, w, a.k, a.c_in, a.c_out, a.c_pad, a.c_out, a.wf, 0, nullptr);
                if (rc) return rc;
            }
        }
    }
    if (e->pad_src && first == 0 && !e->f16) {      // the step's features ride on the first layer's launch (engine_forward)
        int rc = xv_prep_add(J, XV_PREP_PAD, e->pad_src, 1, e->cfg.feat_dim, e->pad_rows, e->c_pad0, e->c_pad0, e->xpad, 0, nullptr);
        if (rc) return rc;
        e->pad_src = nullptr;
    }
    if (A.n) {
        // one memset over the slot range of these layers (tdnn first..F-1 -> slots first..F-1, key layers -> F, F+1: contiguous)
        unsigned *lo = A.out[0], *hi = A.out[0];
        for (int j = 1; j < A.n; ++j) { lo = std::min(lo, A.out[j]); hi = std::max(hi, A.out[j]); }
        if (e->amax_wt_clean) {
            // the forward pass zeroed the whole table in one memset (ahead of this point on `s`, and of the event the side stream waits for)
        } else if (first == 0 && last == 1) {
            XV_CHECK_HIP(hipMemsetAsync(lo, 0, sizeof(uint32_t), s));                    // layer 0 alone (its neighbours belong to the side-stream half)
        } else {
            XV_CHECK_HIP(hipMemsetAsync(lo, 0, (size_t)(hi - lo + 1) * sizeof(uint32_t), s));
        }
        int rc = xv_launch_amax_multi(s, A);
        if (rc) return rc;
    }
    return xv_launch_weight_prep(s, J);
}

int ensure_weights(xv_engine* e, hipStream_t s, bool overlap = false) {
    if (!e->weights_dirty) return 0;
    int rc;
    if (overlap && e->concurrent && e->side) {
        rc = prep_layers(e, s, 0, 1);
        if (rc) return rc;
        XV_CHECK_HIP(hipEventRecord(e->ev_dz, s));              // the update that made the copies stale is ahead of this point on `s`
        XV_CHECK_HIP(hipStreamWaitEvent(e->side, e->ev_dz, 0));
        rc = prep_layers(e, e->side, 1, e->NL);
        if (rc) return rc;
        XV_CHECK_HIP(hipEventRecord(e->ev_prep, e->side));
        e->prep_pending = true;
        rc = xvh_prep_weights(e, e->side);
        if (rc) return rc;
        XV_CHECK_HIP(hipEventRecord(e->ev_lossprep, e->side));
        e->lossprep_pending = true;
    } else {
        rc = prep_layers(e, s, 0, e->NL);
        if (rc) return rc;
        rc = xvh_prep_weights(e, s);
        if (rc) return rc;
    }
    e->weights_dirty = false;
    return 0;
}

// BN (+ReLU) forward of one layer given z
int bn_forward(xv_engine* e, hipStream_t s, XvAffine& a, int rows, bool stats_from_gemm, float* dst_a) {
    const xv_config& c = e->cfg;
    ActScope act(e, a);
    int rc;
    if (e->training && !stats_from_gemm && rows <= XV_BN_SMALL_MAX_ROWS)      // segment-level layers: one launch
        return xv_bn_small_forward(s, a.z, rows, a.c_out, vptr(e, a.v_gamma), vptr(e, a.v_beta), c.bn_epsilon, c.batchnorm_momentum,
                                   a.fused_bn && c.fused_bn_unbiased_moving_var, vptr(e, a.v_mmean), vptr(e, a.v_mvar), a.mean, a.invstd,
                                   a.scale, a.shift, a.has_relu ? 1 : 0, dst_a);
    if (e->training) {
        if (!stats_from_gemm) {
            rc = xv_col_stats(s, a.z, rows, a.c_out, a.ldz, a.bn_part);
            if (rc) return rc;
        }
        rc = xv_bn_finalize(s, a.bn_part, rows, a.c_out, vptr(e, a.v_gamma), vptr(e, a.v_beta), c.bn_epsilon, c.batchnorm_momentum,
                            a.fused_bn && c.fused_bn_unbiased_moving_var, vptr(e, a.v_mmean), vptr(e, a.v_mvar), a.mean, a.invstd,
                            a.scale, a.shift, nullptr, nullptr, nullptr, 1);
    } else {
        rc = xv_bn_inference_scale(s, a.c_out, vptr(e, a.v_gamma), vptr(e, a.v_beta), vptr(e, a.v_mmean), vptr(e, a.v_mvar),
                                   c.bn_epsilon, a.scale, a.shift);
    }
    if (rc) return rc;
    if (!dst_a) return 0;       // the consumer applies scale/shift itself (tdnn5: statistics pooling)
    return xv_bn_apply(s, a.z, rows, a.c_out, a.ldz, a.scale, a.shift, a.has_relu ? 1 : 0, dst_a, a.c_out);
}

// The BN-forward epilogue of a segment-level launch (training mode): z = the launch's result, a_out = act(bn(z))
void skinny_bn_forward(xv_engine* e, XvSkinny& g, XvAffine& a, float* a_out) {
    const xv_config& c = e->cfg;
    ActScope act(e, a);
    g.epi = XV_SK_BN_FWD;
    g.gamma = vptr(e, a.v_gamma); g.beta = vptr(e, a.v_beta); g.eps = c.bn_epsilon; g.momentum = c.batchnorm_momentum;
    g.unbiased = a.fused_bn && c.fused_bn_unbiased_moving_var; g.mmean = vptr(e, a.v_mmean); g.mvar = vptr(e, a.v_mvar);
    g.mean = a.mean; g.invstd = a.invstd; g.scale = a.scale; g.shift = a.shift;
    g.relu = a.has_relu ? 1 : 0; g.slope = a.has_relu ? xv_act_context().slope : nullptr; g.a_out = a_out;
}

// BN (+ activation) forward of a frame-level layer in split precision, given z and the column statistics the GEMM epilogue left in
// bn_part: scale / shift (training: batch statistics and the moving averages; inference: the moving averages) and - out_amax != null -
// the output range, then the fp16 planes the next GEMM reads.  out_amax == null: the fp32 tensor dst_a (the BN+ReLU key of
// att_key_network_type 2, which no GEMM consumes) or nothing (the pooled layer: pooling applies scale / shift itself).
// The column min/max are needed in inference too (they fix the next operand's scale).
int bn_forward_split(xv_engine* e, hipStream_t s, XvAffine& a, int rows, uint32_t* out_amax, float* dst_a) {
    const xv_config& c = e->cfg;
    ActScope act(e, a);
    int rc;
    if (e->training) {
        rc = xv_bn_finalize(s, a.bn_part, rows, a.c_out, vptr(e, a.v_gamma), vptr(e, a.v_beta), c.bn_epsilon, c.batchnorm_momentum,
                            a.fused_bn && c.fused_bn_unbiased_moving_var, vptr(e, a.v_mmean), vptr(e, a.v_mvar), a.mean, a.invstd,
                            a.scale, a.shift, a.zmin, a.zmax, out_amax, 1);
    } else {
        rc = xv_bn_inference_scale(s, a.c_out, vptr(e, a.v_gamma), vptr(e, a.v_beta), vptr(e, a.v_mmean), vptr(e, a.v_mvar),
                                   c.bn_epsilon, a.scale, a.shift);
        if (rc) return rc;
        if (out_amax) rc = xv_bn_output_range(s, a.bn_part, rows, a.c_out, a.scale, a.shift, 1, a.zmin, a.zmax, out_amax);
    }
    if (rc) return rc;
    if (out_amax) return xv_bn_apply_split(s, a.z, rows, a.c_out, a.c_out, a.scale, a.shift, 1, out_amax, a.ah, a.o_ld, (size_t)rows * a.o_ld);
    return dst_a ? xv_bn_apply(s, a.z, rows, a.c_out, a.c_out, a.scale, a.shift, 1, dst_a, a.c_out) : 0;
}

}  // namespace

// Forward of frame-level layer i (a frame layer or an attention key layer) over `segs` chunks of t_in frames: the affine GEMM on the
// output of a.in_layer (the features for tdnn1), then BN (+ activation).  The pooled layer writes no activation (it is applied inside
// the pooling reduction); in split precision a layer a GEMM reads leaves fp16 planes instead of the fp32 tensor.
int xve_layer_forward(xv_engine* e, hipStream_t s, int i, int segs, int t_in) {
    XvAffine& a = e->L[i];
    const int rows = segs * (t_in - a.k + 1);
    const XvAffine* in = a.in_layer < 0 ? nullptr : &e->L[a.in_layer];
    float* dst_a = (i == e->F - 1 && !e->pool_.writes_activation()) ? nullptr : a.a;
    int rc;
    if (e->f16) {
        const unsigned short* xh = in ? in->ah : e->xh;
        const size_t x_stride = (size_t)segs * t_in * (in ? in->o_ld : e->c_pad0);
        const uint32_t* x_amax = in ? e->amax + AMAX_A + in->aslot : e->amax + AMAX_X;
        rc = xv_affine_forward_f16x3(s, xh, x_stride, x_amax, segs, t_in, a.c_pad, a.k, a.wth, a.wth_stride, e->amax + AMAX_WT + a.wslot,
                                     vptr(e, a.v_bias), a.z, a.c_out, a.c_out, a.has_bn ? a.bn_part : nullptr);
        if (rc) return rc;
        if (a.has_bn) rc = bn_forward_split(e, s, a, rows, a.ah ? e->amax + AMAX_A + a.aslot : nullptr, dst_a);
    } else {
        rc = xv_affine_forward(s, in ? in->a : e->xpad, segs, t_in, a.c_pad, a.k, a.wt, vptr(e, a.v_bias), a.z, a.c_out, a.ldz,
                               (a.has_bn && e->training) ? a.bn_part : nullptr, e->ws, e->ws_bytes);
        if (rc) return rc;
        if (a.has_bn) rc = bn_forward(e, s, a, rows, true, dst_a);
    }
    a.rows = rows;
    return rc;
}

namespace {

// The features as the first GEMM's operand: two fp16 planes + a device-side max |x| (split precision: every frame-level operand
// travels that way), or the channel-padded copy - unless that rode on the first layer's weight-copy launch (`padded`)
int input_forward(xv_engine* e, hipStream_t s, const float* features, int b, int t, bool zero_all, bool padded) {
    if (!e->f16) return padded ? 0 : xv_pad_channels(s, features, b * t, e->cfg.feat_dim, e->xpad, e->c_pad0);
    if (!zero_all) XV_CHECK_HIP(hipMemsetAsync(e->amax + AMAX_X, 0, (4 + xv_align(e->F, 4)) * sizeof(uint32_t), s));      // x and every BN+ReLU output slot
    int rc = xv_amax(s, features, (size_t)b * t * e->cfg.feat_dim, e->amax + AMAX_X);
    if (rc) return rc;
    return xv_split_planes(s, features, b * t, e->cfg.feat_dim, e->cfg.feat_dim, e->xh, e->c_pad0, (size_t)b * t * e->c_pad0, e->amax + AMAX_X);
}

// A segment-level layer: dense (+ BatchNorm + activation).  With <= XV_SEGMENT_MAX_ROWS chunks the GEMM, its split-K sum and the
// training-mode BatchNorm are one launch (xv_skinny.hip); otherwise GEMM + slab sum, then the BatchNorm kernels
int segment_forward(xv_engine* e, hipStream_t s, XvAffine& a, const float* x, float* dst_a) {
    const int b = e->B;
    a.rows = b;
    if (e->sk && b <= XV_SEGMENT_MAX_ROWS) {
        XvSkinny g = xve_skinny(e, x, a.c_pad, a.wt, a.c_pad, b, a.c_out, a.c_pad);
        g.bias = vptr(e, a.v_bias); g.C = a.z; g.ldc = a.c_out;
        const bool fused = a.has_bn && e->training;
        if (fused) skinny_bn_forward(e, g, a, dst_a);
        const int rc = xv_launch_skinny(s, g);
        if (rc || fused) return rc;
    } else {
        const int rc = xv_affine_forward(s, x, b, 1, a.c_pad, 1, a.wt, vptr(e, a.v_bias), a.z, a.c_out, a.c_out, nullptr, e->ws, e->ws_bytes);
        if (rc) return rc;
    }
    return a.has_bn ? bn_forward(e, s, a, b, false, dst_a) : 0;
}

// The views of a forward's result: h7 = the last layer's output (its own buffer, or tdnn7's z when nothing follows the affine),
// out = h7 or its l2-normalised, scaled form
int output_forward(xv_engine* e, hipStream_t s) {
    XvAffine& l7 = e->L[e->S1()];
    const int b = e->B;
    int rc = 0;
    e->h7 = (l7.has_bn || l7.has_relu) ? e->h7_buf : l7.z;
    if (!l7.has_bn && l7.has_relu) {      // an activation with no BatchNorm in front (last_layer_no_bn)
        ActScope act(e, l7);
        rc = e->cfg.relu_type != XV_RELU_RELU ? xv_act_small(s, nullptr, l7.z, b, l7.c_out, e->h7_buf)
                                              : xv_relu_backward(s, l7.z, l7.z, (size_t)b * l7.c_out, e->h7_buf);   // z > 0 ? z : 0
        if (rc) return rc;
    }
    e->out = e->h7;
    if (e->cfg.feature_norm) {
        rc = xv_l2_scaling_forward(s, e->h7, b, l7.c_out, e->cfg.feature_scaling_factor, e->out_buf);
        e->out = e->out_buf;
    }
    return rc;
}

int engine_forward(xv_engine* e, void* stream, const float* features, int b, int t, int training, const int32_t* frames) {
    XV_REQUIRE(e && e->V, "engine_forward: engine not bound");
    XV_REQUIRE(b >= 1 && b <= e->cfg.max_batch, "engine_forward: batch %d exceeds capacity %d", b, e->cfg.max_batch);
    XV_REQUIRE(t >= e->min_frames && t <= e->cfg.max_frames, "engine_forward: %d frames outside [%d, %d]", t, e->min_frames, e->cfg.max_frames);
    XV_REQUIRE(e->cfg.max_rows <= 0 || (long)b * t <= (long)e->cfg.max_rows, "engine_forward: %d x %d rows exceed the capacity of %d rows", b, t,
               e->cfg.max_rows);
    XV_REQUIRE(!frames || !training, "engine_forward: per-chunk frame counts are an inference-mode input");
    hipStream_t s = (hipStream_t)stream;
    e->last_stream = s;
    e->B = b; e->T = t; e->training = training;
    // training steps only: there xv_engine_loss_forward always follows and picks up the loss head's event
    // split precision: one memset for every max-|x| slot of the step (input, activations, and - when the weight copies are rebuilt, i.e.
    // on every training step - weights and dz) instead of four ~5 us fill launches along the step
    const bool zero_all = e->f16 && e->weights_dirty;
    if (zero_all) {
        XV_CHECK_HIP(hipMemsetAsync(e->amax, 0, AMAX_SLOTS * sizeof(uint32_t), s));
        e->amax_wt_clean = e->amax_dz_clean = true;
    }
    // fp32: the channel padding of the features is one more job of the first layer's weight-copy launch when that launch happens
    // anyway (every training step); otherwise a launch of its own (input_forward)
    const bool want_pad = !e->f16 && e->weights_dirty;
    e->pad_src = want_pad ? features : nullptr;
    e->pad_rows = b * t;
    int rc = ensure_weights(e, s, training != 0 && e->has_loss());
    e->amax_wt_clean = false;
    const bool padded = want_pad && e->pad_src == nullptr;      // prep_layers took the job
    e->pad_src = nullptr;
    if (rc) return rc;
    rc = input_forward(e, s, features, b, t, zero_all, padded);
    if (rc) return rc;
    const int F = e->F;
    e->Tl[0] = t;
    for (int i = 0; i < F; ++i) {
        if (i == 1) { rc = xve_wait_prep(e, s); if (rc) return rc; }
        rc = xve_layer_forward(e, s, i, b, e->Tl[i]);
        if (rc) return rc;
        e->Tl[i + 1] = e->Tl[i] - e->L[i].k + 1;
    }
    rc = xvp_forward(e, s, b, t, frames);
    if (rc) return rc;
    XvAffine &l6 = e->L[e->S0()], &l7 = e->L[e->S1()];
    rc = segment_forward(e, s, l6, e->pool_.pool, l6.a);
    if (rc) return rc;
    rc = segment_forward(e, s, l7, l6.a, e->h7_buf);
    if (rc) return rc;
    return output_forward(e, s);
}

}  // namespace

extern "C" int xv_engine_forward(xv_engine* e, void* stream, const float* features, int b, int t, int training) {
    return engine_forward(e, stream, features, b, t, training, nullptr);
}
extern "C" int xv_engine_forward_lengths(xv_engine* e, void* stream, const float* features, int b, int t, const int32_t* frames) {
    XV_REQUIRE(frames, "engine_forward_lengths: the per-chunk frame counts are required");
    return engine_forward(e, stream, features, b, t, 0, frames);
}

extern "C" int xv_engine_loss_forward(xv_engine* e, void* stream, const int32_t* labels, int global_step, int with_margin) {
    XV_REQUIRE(e && e->V && e->has_loss(), "engine_loss_forward: engine has no loss head");
    XV_REQUIRE(e->B > 0, "engine_loss_forward: run forward first");
    hipStream_t s = (hipStream_t)stream;
    e->head_.labels_dev = (int32_t*)labels;
    e->head_.with_margin = with_margin;
    int rc = ensure_weights(e, s);
    if (rc) return rc;
    rc = xve_wait_prep(e, s);
    if (rc) return rc;
    rc = xve_wait_lossprep(e, s);
    if (rc) return rc;
    return xvh_loss_forward(e, s, labels, global_step);
}

// regularization_loss, trainer.py:357-358.  It does not feed any gradient (the L2 term is added
// analytically in the weight-gradient reduce), so it is only evaluated when the host asks for it
// (the reference fetches it on logging steps only, trainer.py:485-499).
int xve_reg_loss(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    XV_CHECK_HIP(hipMemsetAsync(e->scalars + 1, 0, sizeof(float), s));
    for (int i = 0; i < e->NL; ++i) {
        int rc = xv_sumsq_ordered(s, vptr(e, e->L[i].v_kernel), e->vars[e->L[i].v_kernel].count, 0.5f * c.weight_l2_regularizer, e->scalars + 1, (float*)e->ws);
        if (rc) return rc;
    }
    int rc = xvp_reg_loss(e, s);
    if (rc) return rc;
    rc = xvh_reg_loss(e, s);
    if (rc) return rc;
    e->reg_valid = true;
    return 0;
}
