// Engine, backward: the stream protocol - the weight-gradient side streams, the dz ring whose slots the data-gradient chain hands to
// them, the join, the stage events - then the backward of one layer in fp32 and in split precision, and the four stages of a pass
// (0: loss head (xv_engine_head.hip) + segment layers, 1: the pooling layer (xv_engine_pool.hip) + the last two frame layers, 2 and 3: the
// frame layers below; build_variables lays the gradient buffer out so that each stage finishes a contiguous slice).
#include "xv_engine.h"

// Make `waiter` wait for everything enqueued so far on `signaller` (through `ev`).
int xve_chain(hipStream_t signaller, hipStream_t waiter, hipEvent_t ev) {
    XV_CHECK_HIP(hipEventRecord(ev, signaller));
    XV_CHECK_HIP(hipStreamWaitEvent(waiter, ev, 0));
    return 0;
}

namespace {

using ZRing = xv_engine::ZRing;

// All weight-gradient work enqueued on the side streams so far becomes visible to `s` - through ONE wait on `s`: the side stream is in
// order, so an event recorded on it now covers every dz slot's event, and the loss head's stream is joined into the side stream first.
// (tools/sync_cost_probe.cpp, profiles/r04_sync_cost.txt: in a chain of 10 us kernels a wait for another stream's fresh event costs the
// waiting stream 4 us, a record 3 us, record + the other stream's wait 5.6 us; in the step the difference between three waits and one is
// within the noise of a same-box A/B - as is carrying the hand-over events on the producing kernels' completion signals
// (hipExtLaunchKernel's stopEvent, 1.5 us in the probe), which was built, verified and taken out again.)
int join_side(xv_engine* e, hipStream_t s) {
    bool any = e->side_dirty;
    e->side_dirty = false;
    e->z_taken = 0;
    for (int r = 0; r < 2; ++r)
        for (int i = 0; i < XV_Z_SLOTS; ++i) {
            any = any || e->zr[r].pending[i];
            e->zr[r].pending[i] = false;
        }
    if (e->lw_pending) {
        if (e->side) XV_CHECK_HIP(hipStreamWaitEvent(e->side, e->ev_lw, 0));
        else XV_CHECK_HIP(hipStreamWaitEvent(s, e->ev_lw, 0));
        any = any || e->side;
        e->lw_pending = false;
    }
    if (any && e->side) {
        XV_CHECK_HIP(hipEventRecord(e->ev_join, e->side));
        XV_CHECK_HIP(hipStreamWaitEvent(s, e->ev_join, 0));
    }
    return 0;
}

// The two rings (xv_engine.h, "dz ping-pong state"): the frame-level layers' dz - fp16 planes `dzh` in split precision - and the
// fp32 dz in `bufZ` of this mode: every layer's in fp32 (the same ring), the segment layers' and the key gradient in split precision
ZRing& frame_ring(xv_engine* e) { return e->zr[0]; }
ZRing& f32_ring(xv_engine* e) { return e->zr[e->f16 ? 1 : 0]; }

// The dz-ring protocol, first half: the ring's current slot, once the weight gradient that last read it (two layers up, side stream)
// has finished.  -1: the wait could not be enqueued.
int ring_take(xv_engine* e, hipStream_t s, ZRing& zr) {
    const int zi = zr.cur;
    if (e->z_private && e->z_taken >= zr.n && join_side(e, s)) return -1;      // (a caller that never finishes a backward pass)
    if (zr.pending[zi]) {                       // WAR
        if (hipStreamWaitEvent(s, zr.ev[zi], 0) != hipSuccess) return -1;
        zr.pending[zi] = false;
    }
    return zi;
}

// ... second half: the slot taken last now holds a dz; launch(stream, workspace) enqueues the weight gradient that reads it, and the ring
// moves on.  The weight gradient only shares dz with the data-gradient chain, so it goes to the side stream behind everything on `s`
// (ev_dz): its workgroups fill the CUs that the tail of the data-gradient GEMM (and the small BN kernels of the next layer) leave idle.
// The slot's event says when it may be rewritten; with a slot per layer (z_private) none is taken again before the join at the end of
// the step, so nothing is recorded.  In line on `s` instead:
//  - first: the first layer is the end of the chain: nothing is left on `s` to overlap with, and the side stream is still busy with the
//    layer above's weight gradient - its own (small) weight gradient finishes sooner in line on `s`, beside that one (round-2
//    timeline: 166 us of MFMA-idle tail behind tdnn2's weight gradient: tdnn1's, two slab sums, the update)
//  - zr == nullptr: dz is no ring slot but the caller's own buffer: everything stays in order, and no ring moves
//  - xv_engine_set_concurrency(0)
template <class Launch>
int ring_give(xv_engine* e, hipStream_t s, ZRing* zr, bool first, Launch launch) {
    const bool conc = e->concurrent && zr && !first;
    int rc;
    if (conc) {
        rc = xve_chain(s, e->side, e->ev_dz);
        if (rc) return rc;
    }
    rc = launch(conc ? e->side : s, conc ? e->ws_side : e->ws);
    if (rc) return rc;
    if (conc) {
        if (e->z_private) { e->side_dirty = true; ++e->z_taken; }
        else {
            XV_CHECK_HIP(hipEventRecord(zr->ev[zr->cur], e->side));
            zr->pending[zr->cur] = true;
        }
    }
    if (zr) zr->cur = (zr->cur + 1) % zr->n;
    return 0;
}

}  // namespace

// a slot of bufZ (nullptr: ring_take failed)
float* xve_take_dz(xv_engine* e, hipStream_t s) {
    const int zi = ring_take(e, s, f32_ring(e));
    return zi < 0 ? nullptr : e->bufZ[zi];
}

namespace {

// dz of layer `a` (fp32 path) from the gradient w.r.t. its output: BN (+activation) backward, the activation alone, or da itself.
// *ring: dz was written into the ring's current slot (take_dz) - the caller's weight gradient then owns the slot.
int layer_dz(xv_engine* e, hipStream_t s, XvAffine& a, const float* da, int segs, int t_out, int pad, const float* act_out,
             const float** dz_out, bool* ring) {
    const xv_config& c = e->cfg;
    const int lidx = (int)(&a - &e->L[0]);
    ActScope act(e, a);
    int rc;
    *ring = true;
    float* Z = xve_take_dz(e, s);
    XV_REQUIRE_SLOT(Z);
    if (!da) {       // tdnn5: the upstream gradient is the statistics-pooling backward of (pool, d pool)
        XV_REQUIRE(lidx == e->F - 1 && a.has_bn, "engine_backward: only the last frame layer takes its gradient from the pooling layer");
        rc = xv_bn_backward_f32(s, xvp_upstream(e), a.z, e->B * e->Tl[e->F], 1, a.c_out, vptr(e, a.v_gamma), a.mean, a.invstd, a.scale, a.shift, 1,
                                0, Z, a.ldz, gptr(e, a.v_gamma), gptr(e, a.v_beta), gptr(e, a.v_bias), e->ws, e->ws_bytes);
    } else if (a.has_bn && pad == 0 && segs * t_out <= XV_BN_SMALL_MAX_ROWS && !is_frame(e, lidx)) {      // segment-level layers: one launch
        rc = xv_bn_small_backward(s, da, a.z, segs * t_out, a.c_out, vptr(e, a.v_gamma), a.mean, a.invstd, a.scale, a.shift,
                                  a.has_relu ? 1 : 0, Z, gptr(e, a.v_gamma), gptr(e, a.v_beta), gptr(e, a.v_bias));
    } else if (a.has_bn) {
        rc = xv_bn_relu_backward(s, da, a.z, segs, t_out, a.c_out, vptr(e, a.v_gamma), a.mean, a.invstd, a.scale, a.shift,
                                 a.has_relu ? 1 : 0, pad, Z, gptr(e, a.v_gamma), gptr(e, a.v_beta), gptr(e, a.v_bias), e->ws, e->ws_bytes);
    } else if (a.has_relu && c.relu_type != XV_RELU_RELU) {       // activation without a BN in front (tdnn7, last_layer_no_bn): needs the pre-activation
        rc = xv_act_small(s, da, a.z, segs * t_out, a.c_out, Z);
    } else if (a.has_relu) {
        rc = xv_relu_backward(s, da, act_out, (size_t)segs * t_out * a.c_out, Z);
    } else {
        *dz_out = da;
        *ring = (da == Z);       // the caller wrote d(output) into the ring's slot itself (attention key gradient)
        return 0;
    }
    *dz_out = Z;
    return rc;
}

// the launches of one layer's weight (and, without a BatchNorm, bias) gradient on `q` with workspace `wws`
int layer_wgrad_on(xv_engine* e, hipStream_t q, void* wws, XvAffine& a, const float* x, const float* dz, int segs, int t_in, int pad) {
    const xv_config& c = e->cfg;
    const int t_out = t_in - a.k + 1;
    const int seg_pitch = t_out + 2 * pad;
    int rc = xv_affine_wgrad_ld(q, x, segs, t_in, a.c_pad, a.k, a.c_in, dz, a.ldz, seg_pitch, pad, a.c_out, vptr(e, a.v_kernel),
                                c.weight_l2_regularizer, gptr(e, a.v_kernel), wws, e->ws_bytes);
    if (rc) return rc;
    if (!a.has_bn)       // a bias in front of a BN gets its (zero + rounding noise) gradient from the BN backward
        rc = xv_colsum(q, dz, segs * seg_pitch, a.c_out, a.c_out, gptr(e, a.v_bias), wws, e->ws_bytes);
    return rc;
}

// Weight (and, without a BN, bias) gradient of layer `a` from (x, dz), handed over through the fp32 ring (ring: dz is its current slot)
int layer_wgrad(xv_engine* e, hipStream_t s, XvAffine& a, const float* x, const float* dz, int segs, int t_in, int pad, bool ring,
                bool first = false) {
    // [measured, round 4, same box, variant builds] the LAST weight-gradient launches of the side stream (tdnn2's; tdnn2-3's; all four) as 768
    // rectangles instead of a full round - so that the BatchNorm backward of tdnn1, which waits 250-300 us for slots beside tdnn2's weight
    // gradient at the very end of the step, finds a free slot per CU: S1 5.22 -> 5.29 / 5.24 / 5.24 ms, 64 x U{200..400} 4.30 -> 4.33 / 4.34 /
    // 4.35 ms.  The full round stays.
    return ring_give(e, s, ring ? &f32_ring(e) : nullptr, first,
                     [&](hipStream_t q, void* wws) { return layer_wgrad_on(e, q, wws, a, x, dz, segs, t_in, pad); });
}

int layer_backward_f16(xv_engine* e, hipStream_t s, int li, const float* da, int segs, int t_in, float* dx);

}  // namespace

// backward of one affine(+BN+ReLU) layer.  da: gradient w.r.t. the layer OUTPUT (after BN/ReLU),
// dense [segs*t_out][c_out].  x/t_in: the layer input view.  Writes parameter gradients and, if
// dx != nullptr, the gradient w.r.t. the layer input ([segs*t_in][c_in]); dx == nullptr marks the first layer.
int xve_layer_backward(xv_engine* e, hipStream_t s, XvAffine& a, const float* da, const float* x, int segs, int t_in, float* dx,
                       const float* act_out) {
    const int t_out = t_in - a.k + 1;
    const int pad = (dx && a.k > 1) ? a.k - 1 : 0;
    const int lidx = (int)(&a - &e->L[0]);
    if (e->f16 && is_frame(e, lidx)) return layer_backward_f16(e, s, lidx, da, segs, t_in, dx);
    const float* dz = nullptr;
    bool ring = false;
    int rc = layer_dz(e, s, a, da, segs, t_out, pad, act_out, &dz, &ring);
    if (rc) return rc;
    rc = layer_wgrad(e, s, a, x, dz, segs, t_in, pad, ring, dx == nullptr);
    if (rc) return rc;
    if (dx) {
        const float* wf = a.k > 1 ? a.wf : vptr(e, a.v_kernel);
        rc = xv_affine_dgrad_ld(s, dz, a.ldz, segs, t_out, a.c_out, a.k, wf, dx, a.c_in, e->ws, e->ws_bytes);
        if (rc) return rc;
    }
    return 0;
}

namespace {

// Split-precision backward of a frame layer: dz is written once as fp16 planes (padded layout) and feeds both the
// weight gradient (TN, side stream; A operand = the planes the forward pass already consumed) and the data gradient
// (NT, tap-flipped weight planes).  Only what is specific to planes is here; the slots come and go as in layer_backward.
int layer_backward_f16(xv_engine* e, hipStream_t s, int li, const float* da, int segs, int t_in, float* dx) {
    XvAffine& a = e->L[li];
    const xv_config& c = e->cfg;
    ActScope act(e, a);
    const int t_out = t_in - a.k + 1;
    const int pad = (dx && a.k > 1) ? a.k - 1 : 0;
    const int zi = ring_take(e, s, frame_ring(e));
    XV_REQUIRE_SLOT(zi >= 0);
    unsigned short* Z = e->dzh[zi];
    uint32_t* zamax = e->amax + AMAX_DZ + a.wslot;
    const int seg_pitch = t_out + 2 * pad;
    const size_t zstride = (size_t)segs * seg_pitch * a.o_ld;
    XV_REQUIRE(zstride <= e->dzh_halfs, "engine_backward: dz plane buffer too small");
    int rc;
    if (da && !a.has_bn) {      // att_key1: `da` already is dz (fp32): planes + the bias gradient straight from it
        XV_REQUIRE(pad == 0 && !a.has_relu, "engine_backward: a frame layer without BN is the attention key layer");
        rc = xv_amax(s, da, (size_t)segs * t_out * a.c_out, zamax);
        if (rc) return rc;
        rc = xv_split_planes(s, da, segs * t_out, a.c_out, a.c_out, Z, a.o_ld, zstride, zamax);
        if (rc) return rc;
        rc = xv_colsum(s, da, segs * t_out, a.c_out, a.c_out, gptr(e, a.v_bias), e->ws, e->ws_bytes);
    } else {
        XvBnUpstream up = {};
        up.da = da;
        if (!da) {       // tdnn5
            XV_REQUIRE(li == e->F - 1, "engine_backward: only the last frame layer takes its gradient from the pooling layer");
            up = xvp_upstream(e);
        } else if (e->bwd_part_layer == li && e->bwd_part_chunks == xv_cdiv(segs * t_out, XV_TILE_M)) {
            // the GEMM that produced `da` already reduced it against this layer's z (xv_affine_dgrad_bnstats_f16x3)
            up.ext_part = e->bwd_part; up.ext_chunks = e->bwd_part_chunks;
        }
        // zero_amax = false: the dz slots were zeroed at the start of this backward pass
        rc = xv_bn_backward_split(s, up, a.z, da ? segs : e->B * e->Tl[e->F], da ? t_out : 1, a.c_out, vptr(e, a.v_gamma), a.mean, a.invstd,
                                  a.scale, a.shift, a.zmin, a.zmax, 1, pad, Z, a.o_ld, zstride, zamax, false, gptr(e, a.v_gamma),
                                  gptr(e, a.v_beta), gptr(e, a.v_bias), e->ws, e->ws_bytes);
    }
    e->bwd_part_layer = -1;
    if (rc) return rc;
    // operand planes of this layer's input: the feature planes for tdnn1, the producing layer's BN+ReLU planes otherwise
    const int in = a.in_layer;
    const unsigned short* xin = in < 0 ? e->xh : e->L[in].ah;
    const int xin_rows = in < 0 ? e->B * e->Tl[0] : e->L[in].rows;
    const uint32_t* xin_amax = in < 0 ? e->amax + AMAX_X : e->amax + AMAX_A + e->L[in].aslot;
    rc = ring_give(e, s, &frame_ring(e), dx == nullptr, [&](hipStream_t q, void* wws) {
        return xv_affine_wgrad_f16x3(q, xin, (size_t)xin_rows * a.c_pad, xin_amax, segs, t_in, a.c_pad, a.k, a.c_in, Z, zstride, zamax, seg_pitch,
                                     pad, a.o_ld, a.c_out, vptr(e, a.v_kernel), c.weight_l2_regularizer, gptr(e, a.v_kernel), wws, e->ws_bytes);
    });
    if (rc) return rc;
    if (dx) {
        // [measured, round 1] folding the producing layer's BN-backward reductions into this GEMM's epilogue (xv_affine_dgrad_bnstats_f16x3,
        // kept parity-tested at op level) is not used: the epilogue's extra z-tile reads cost each data-gradient GEMM 50-60 us at S1, the
        // reduce kernels they replace 37 us each (3.17 vs 3.03 ms/step)
        rc = xv_affine_dgrad_f16x3(s, Z, zstride, zamax, segs, t_out, a.o_ld, a.k, a.wfh, a.wfh_stride, e->amax + AMAX_WT + a.wslot, dx, a.c_in);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

// The BN-backward epilogue of a segment-level launch: the launch's result is d a of layer `a`; C = its dz, and the BN / bias gradients
void xve_skinny_bn_backward(xv_engine* e, XvSkinny& g, XvAffine& a, float* dz) {
    ActScope act(e, a);
    const XvActContext ac = xv_act_context();
    g.epi = XV_SK_BN_BWD; g.C = dz; g.ldc = a.c_out;
    g.z = a.z; g.gamma = vptr(e, a.v_gamma); g.mean = a.mean; g.invstd = a.invstd; g.scale = a.scale; g.shift = a.shift;
    g.relu = a.has_relu ? 1 : 0; g.slope = a.has_relu ? ac.slope : nullptr; g.dalpha = (a.has_relu && ac.slope) ? ac.dalpha : nullptr;
    g.dgamma = gptr(e, a.v_gamma); g.dbeta = gptr(e, a.v_beta); g.dbias = gptr(e, a.v_bias);
}

namespace {

// Stage 0: the loss head and the two segment-level layers, down to d pool (d_small0).  The pooling backward itself is evaluated
// inside the last frame layer's BN backward (stage 1) from (pool, d pool): its d a is never written.
int backward_segment(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    const int b = e->B;
    if (e->f16 && !e->amax_dz_clean) XV_CHECK_HIP(hipMemsetAsync(e->amax + AMAX_DZ, 0, xv_align(e->F + 2, 4) * sizeof(uint32_t), s));   // every layer's dz scale slot
    e->amax_dz_clean = false;
    int rc = xvh_wgrad(e, s);
    if (rc) return rc;
    // d out (with tdnn7's BN backward on the same launch where the head can fuse it), then the ring loss's d r
    XvAffine &l6 = e->L[e->S0()], &l7 = e->L[e->S1()];
    const bool sk = e->sk && b <= XV_SEGMENT_MAX_ROWS;
    float* dz7_fused = nullptr;
    rc = xvh_dout(e, s, sk, &dz7_fused);
    if (rc) return rc;
    const bool fuse7 = dz7_fused != nullptr;
    rc = xvh_ring_grad(e, s);
    if (rc) return rc;
    const float* d = e->d_small0;      // d h7 (not there when tdnn7's BN backward rode on the d-out launch)
    if (c.feature_norm) {
        rc = xv_l2_scaling_backward(s, e->h7, d, b, e->Lout, c.feature_scaling_factor, e->d_small1);
        if (rc) return rc;
        d = e->d_small1;
    }
    if (!sk) {      // tdnn7 -> d a6 (into bufD), tdnn6 -> d pool
        rc = xve_layer_backward(e, s, l7, d, l6.a, b, 1, e->bufD, e->h7);
        if (rc) return rc;
        return xve_layer_backward(e, s, l6, e->bufD, e->pool_.pool, b, 1, e->d_small0, nullptr);
    }
    // tdnn7's dz (already there when fused), its weight gradient on the side stream
    const float* dz7 = dz7_fused;
    bool ring7 = true;
    if (!fuse7) {
        rc = layer_dz(e, s, l7, d, b, 1, 0, e->h7, &dz7, &ring7);
        if (rc) return rc;
    }
    // [measured, round 6, profiles/r06_scheduled_update.txt] both segment layers' weight gradients behind ONE event record (after dz6) on the
    // loss head's stream instead of a record each: S1 +0.3 ... +0.5 %, 64 x U +0.2 %; with no record of their own (launched with the last
    // frame layer's hand-over) +0.8 % / +0.4 % - the packets on the compute stream are not what this chain costs
    rc = layer_wgrad(e, s, l7, l6.a, dz7, b, 1, 0, ring7);
    if (rc) return rc;
    // d a6 = dz7 . W7^T and tdnn6's BatchNorm (+ activation) backward in one launch -> dz6
    float* dz6 = xve_take_dz(e, s);
    XV_REQUIRE_SLOT(dz6);
    XV_REQUIRE(l6.has_bn, "engine_backward: the first segment-level layer has a BatchNorm (tdnn.py:147-163)");
    XvSkinny g = xve_skinny(e, dz7, l7.c_out, vptr(e, l7.v_kernel), l7.c_out, b, l7.c_in, l7.c_out);
    xve_skinny_bn_backward(e, g, l6, dz6);
    rc = xv_launch_skinny(s, g);
    if (rc) return rc;
    rc = layer_wgrad(e, s, l6, e->pool_.pool, dz6, b, 1, 0, true);
    if (rc) return rc;
    // d pool = dz6 . W6^T
    g = xve_skinny(e, dz6, l6.c_out, vptr(e, l6.v_kernel), l6.c_out, b, l6.c_in, l6.c_out);
    g.C = e->d_small0; g.ldc = l6.c_in;
    return xv_launch_skinny(s, g);
}

// backward of frame layer i: a context layer sees chunks of Tl[i] frames, a dense layer one "chunk" per frame
int frame_backward(xv_engine* e, hipStream_t s, int i, const float* da) {
    XvAffine& a = e->L[i];
    const float* x = i > 0 ? e->L[i - 1].a : e->xpad;
    float* dx = i > 0 ? e->bufD : nullptr;
    if (a.k > 1) return xve_layer_backward(e, s, a, da, x, e->B, e->Tl[i], dx, nullptr);
    return xve_layer_backward(e, s, a, da, x, e->B * e->Tl[i + 1], 1, dx, nullptr);
}

// End of a backward stage.  Joining: `s` waits for the side stream, so the stage's gradients are complete on `s` (a collective
// enqueued on `s` next sees them) - but `s` then also stalls until the weight gradients have drained, which costs the overlap
// of the next stage's data-gradient chain with them (0.2 ms/step at S1).  Deferred: both streams only record an event; whoever
// consumes the slice waits for the pair (xv_engine_stage_wait) on its own stream.
int end_stage(xv_engine* e, hipStream_t s, int stage, bool defer) {
    if (!defer) return join_side(e, s);
    const bool last = stage == XV_BWD_STAGES - 1;
    if (last) {                       // the optimiser step follows on `s`: join here, the event on `s` then covers both streams
        int rc = join_side(e, s);
        if (rc) return rc;
    }
    XV_CHECK_HIP(hipEventRecord(e->ev_stage[stage][0], s));
    if (stage == 0) e->stage_lw = e->lw_pending;      // the loss head's weight gradient (third stream) belongs to this slice
    e->stage_side[stage] = !last && e->concurrent && e->side;
    if (e->stage_side[stage]) XV_CHECK_HIP(hipEventRecord(e->ev_stage[stage][1], e->side));
    return 0;
}
int engine_backward(xv_engine* e, void* stream, int stage, bool defer) {
    XV_REQUIRE(e && e->V && e->G, "engine_backward: gradient buffer not bound");
    XV_REQUIRE(e->training && e->head_.labels_dev, "engine_backward: needs a training forward + loss_forward first");
    XV_REQUIRE(stage >= -1 && stage < XV_BWD_STAGES, "engine_backward: bad stage %d", stage);
    hipStream_t s = (hipStream_t)stream;
    const int F = e->F;
    const int lo = F >= 4 ? 2 : 1;    // first layer of stage 2 (build_variables: stage ranges)
    int rc;
    if (stage == -1 || stage == 0) {
        rc = backward_segment(e, s);
        if (rc) return rc;
        if (stage == 0) { rc = end_stage(e, s, 0, defer); if (rc) return rc; }
    }
    if (stage == -1 || stage == 1) {
        const float* da = nullptr;
        rc = xvp_backward(e, s, &da);
        if (rc) return rc;
        rc = frame_backward(e, s, F - 1, da);                 // last frame layer (da = pooling backward: materialised, or nullptr = inside its BN backward)
        if (rc) return rc;
        rc = xvp_backward_join(e, s);
        if (rc) return rc;
        rc = frame_backward(e, s, F - 2, e->bufD);
        if (rc) return rc;
        if (stage == 1) { rc = end_stage(e, s, 1, defer); if (rc) return rc; }
    }
    if (stage == -1 || stage == 2) {
        for (int i = F - 3; i >= lo; --i) {
            rc = frame_backward(e, s, i, e->bufD);
            if (rc) return rc;
        }
        if (stage == 2) { rc = end_stage(e, s, 2, defer); if (rc) return rc; }
    }
    if (stage == -1 || stage == 3) {
        for (int i = lo - 1; i >= 0; --i) {
            rc = frame_backward(e, s, i, e->bufD);
            if (rc) return rc;
        }
        rc = end_stage(e, s, XV_BWD_STAGES - 1, defer);       // end of the backward pass: every gradient is visible to `stream`
        if (rc) return rc;
    }
    return 0;
}
}  // namespace

extern "C" int xv_engine_backward(xv_engine* e, void* stream, int stage) { return engine_backward(e, stream, stage, false); }

extern "C" int xv_engine_backward_async(xv_engine* e, void* stream, int stage) {
    XV_REQUIRE(stage >= 0 && stage < XV_BWD_STAGES, "engine_backward_async: stage %d is not one of 0..%d", stage, XV_BWD_STAGES - 1);
    return engine_backward(e, stream, stage, true);
}

extern "C" int xv_engine_stage_wait(xv_engine* e, void* waiter_stream, int stage) {
    XV_REQUIRE(e && stage >= 0 && stage < XV_BWD_STAGES, "engine_stage_wait: bad arguments");
    hipStream_t w = (hipStream_t)waiter_stream;
    XV_CHECK_HIP(hipStreamWaitEvent(w, e->ev_stage[stage][0], 0));
    if (e->stage_side[stage]) XV_CHECK_HIP(hipStreamWaitEvent(w, e->ev_stage[stage][1], 0));
    if (stage == 0 && e->stage_lw) XV_CHECK_HIP(hipStreamWaitEvent(w, e->ev_lw, 0));
    return 0;
}
