// Engine, backward: the stream protocol - the weight-gradient side streams, the dz ring whose slots the data-gradient chain hands to
// them, the join, the stage events - then the backward of one layer in fp32 and in split precision, the loss head's weight gradient,
// and the four stages of a pass (0: loss head + segment layers, 1: attention keys + the last two frame layers, 2 and 3: the frame layers
// below; build_variables lays the gradient buffer out so that each stage finishes a contiguous slice).
#include "xv_engine.h"

namespace {

using ZRing = xv_engine::ZRing;

// Make `waiter` wait for everything enqueued so far on `signaller` (through `ev`).
int chain(hipStream_t signaller, hipStream_t waiter, hipEvent_t ev) {
    XV_CHECK_HIP(hipEventRecord(ev, signaller));
    XV_CHECK_HIP(hipStreamWaitEvent(waiter, ev, 0));
    return 0;
}

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
#define XV_REQUIRE_SLOT(cond) XV_REQUIRE(cond, "engine_backward: waiting for a dz slot failed")

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
        rc = chain(s, e->side, e->ev_dz);
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

// a slot of bufZ (nullptr: ring_take failed)
float* take_dz(xv_engine* e, hipStream_t s) {
    const int zi = ring_take(e, s, f32_ring(e));
    return zi < 0 ? nullptr : e->bufZ[zi];
}

// The upstream gradient of the last frame layer (tdnn5): the (attention-weighted) statistics-pooling backward of (pool, d pool)
XvBnUpstream pooled_upstream(const xv_engine* e) {
    XvBnUpstream up = {};
    up.pool_out = e->pool; up.dpool = e->d_small0; up.pool_t = e->Tl[e->F]; up.weights = e->att ? e->att_w : nullptr;
    if (e->pool_closed_form) { up.wpos = e->pool_wpos; up.pamax = e->pool_amax; }
    return up;
}

// dz of layer `a` (fp32 path) from the gradient w.r.t. its output: BN (+activation) backward, the activation alone, or da itself.
// *ring: dz was written into the ring's current slot (take_dz) - the caller's weight gradient then owns the slot.
int layer_dz(xv_engine* e, hipStream_t s, XvAffine& a, const float* da, int segs, int t_out, int pad, const float* act_out,
             const float** dz_out, bool* ring) {
    const xv_config& c = e->cfg;
    const int lidx = (int)(&a - &e->L[0]);
    ActScope act(e, a);
    int rc;
    *ring = true;
    float* Z = take_dz(e, s);
    XV_REQUIRE_SLOT(Z);
    if (!da) {       // tdnn5: the upstream gradient is the statistics-pooling backward of (pool, d pool)
        XV_REQUIRE(lidx == e->F - 1 && a.has_bn, "engine_backward: only the last frame layer takes its gradient from the pooling layer");
        rc = xv_bn_backward_f32(s, pooled_upstream(e), a.z, e->B * e->Tl[e->F], 1, a.c_out, vptr(e, a.v_gamma), a.mean, a.invstd, a.scale, a.shift, 1,
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

// backward of one affine(+BN+ReLU) layer.  da: gradient w.r.t. the layer OUTPUT (after BN/ReLU),
// dense [segs*t_out][c_out].  x/t_in: the layer input view.  Writes parameter gradients and, if
// dx != nullptr, the gradient w.r.t. the layer input ([segs*t_in][c_in]); dx == nullptr marks the first layer.
int layer_backward(xv_engine* e, hipStream_t s, XvAffine& a, const float* da, const float* x, int segs, int t_in, float* dx,
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
            up = pooled_upstream(e);
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

// d wn = out^T . dlogits and the gradient through l2_normalize: on a stream of its own (it only reads dlogits / out / wn, which
// the main chain never rewrites during backward), started before anything else of the backward pass.  [measured, same box]
// on the weight-gradient stream, BEHIND the segment layers' weight gradients, it cost fp32 mode 0.2 ms/step (it then ran beside
// the big data-gradient GEMMs, 10x slower, with the frame layers' weight gradients queued behind it); IN FRONT of them the
// last frame layer's BN backward waited ~80 us for the dz slot tdnn7's weight gradient still had to read; on its own stream but
// launched at the END of this stage (it has 3 ms of slack, and d out runs 23 instead of 49 us without it alongside) it again
// costs fp32 0.24 ms: its many-workgroup TN kernel then competes with the first big data-gradient GEMMs
// [measured, round 3] started right BEHIND the d-out launch instead of in front of it: no difference (5.36 / 4.42 / 12.70 ms at S1 / 64 x 300 / S5 either way)
// [measured, round 4, same box, variant builds] started behind the d-POOL launch (the chain d out -> d tdnn6 -> d pool then runs with
// the chip to itself: d out 23 instead of 49 us, one event instead of three): S1 5.22 -> 5.40 ms, 64 x U{200..400} 4.32 -> 4.41 ms -
// with the segment layers' weight gradients moved behind it as well 5.41 / 4.44 ms.  Its slab sum and normalisation kernels then run
// beside the first big GEMMs and crawl (236 / 113 / 247 us for 15 / 33 / 18), and everything queued behind them starts late.
int loss_head_wgrad(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    const int b = e->B;
    int rc = 0;
    hipStream_t ss = e->concurrent ? e->side2 : s;
    void* lws = e->concurrent ? e->ws_side2 : e->ws_side;
    if (e->concurrent) {
        rc = chain(s, ss, e->ev_dz);
        if (rc) return rc;
    }
    XvGemmTN w = {};
    w.A = e->out; w.lda = e->Lout; w.a_rps = b; w.a_pitch = b;
    w.B = e->dlogits; w.ldb = e->ldl; w.b_rps = b; w.b_pitch = b;
    w.M = e->Lout; w.N = e->ldl; w.R = b;
    w.direct = 1;
    w.splits = xv_tn_splits_direct(w.M, w.N, w.R);
    XV_REQUIRE(w.splits == 1 || (size_t)w.splits * w.M * w.N * sizeof(float) <= e->ws_bytes, "engine_backward: workspace too small for the loss weight gradient");
    // unsplit (xv_tn_plan: a short reduction over many tiles): the one "slab" IS d wn [Lout][ldl] - no slab sum
    w.P = w.splits == 1 ? e->dwn : (float*)lws;
    rc = xv_launch_gemm_tn(ss, w);
    if (rc) return rc;
    if (w.splits > 1) {
        rc = xv_launch_wgrad_reduce(ss, w.P, w.splits, 1, e->Lout, e->Lout, e->ldl, e->ldl, nullptr, 0, 0.f, e->dwn, e->ldl);
        if (rc) return rc;
    }
    if (e->with_margin && c.aux_mhe) {
        rc = xv_mhe_add_grad(ss, e->dwn, e->Lout, e->N, e->ldl, e->mhe_coef, e->mhe_counts);
        if (rc) return rc;
    }
    rc = xv_loss_weight_backward(ss, e->dwn, e->ldl, e->wn, e->ldl, e->inv_norm, vptr(e, e->v_loss_kernel), e->Lout, e->N,
                                 c.loss_kind != XV_LOSS_SOFTMAX, xve_output_l2(c), gptr(e, e->v_loss_kernel), lws, e->ws_bytes);
    if (rc) return rc;
    if (e->v_loss_bias >= 0) {
        rc = xv_colsum(ss, e->dlogits, b, e->N, e->ldl, gptr(e, e->v_loss_bias), lws, e->ws_bytes);
        if (rc) return rc;
    }
    if (e->concurrent) {
        XV_CHECK_HIP(hipEventRecord(e->ev_lw, ss));
        e->lw_pending = true;
    }
    return 0;
}

// The BN-backward epilogue of a segment-level launch: the launch's result is d a of layer `a`; C = its dz, and the BN / bias gradients
void skinny_bn_backward(xv_engine* e, XvSkinny& g, XvAffine& a, float* dz) {
    ActScope act(e, a);
    const XvActContext ac = xv_act_context();
    g.epi = XV_SK_BN_BWD; g.C = dz; g.ldc = a.c_out;
    g.z = a.z; g.gamma = vptr(e, a.v_gamma); g.mean = a.mean; g.invstd = a.invstd; g.scale = a.scale; g.shift = a.shift;
    g.relu = a.has_relu ? 1 : 0; g.slope = a.has_relu ? ac.slope : nullptr; g.dalpha = (a.has_relu && ac.slope) ? ac.dalpha : nullptr;
    g.dgamma = gptr(e, a.v_gamma); g.dbeta = gptr(e, a.v_beta); g.dbias = gptr(e, a.v_bias);
}

// Stage 0: the loss head and the two segment-level layers, down to d pool (d_small0).  The pooling backward itself is evaluated
// inside the last frame layer's BN backward (stage 1) from (pool, d pool): its d a is never written.
int backward_segment(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    const int b = e->B;
    if (e->f16 && !e->amax_dz_clean) XV_CHECK_HIP(hipMemsetAsync(e->amax + AMAX_DZ, 0, xv_align(e->F + 2, 4) * sizeof(uint32_t), s));   // every layer's dz scale slot
    e->amax_dz_clean = false;
    int rc = e->pair ? 0 : loss_head_wgrad(e, s);
    if (rc) return rc;
    // d out = dlogits . wn^T   (pad column of both is zero, so K = ldl is exact), + the gradient through ||out|| (loss.py:122,147).
    // Fused form (xv_skinny.hip): one launch, and with a BatchNorm in tdnn7 and no l2_scaling in between, tdnn7's BN backward too
    XvAffine &l6 = e->L[e->S0()], &l7 = e->L[e->S1()];
    const bool sk = e->sk && b <= XV_SEGMENT_MAX_ROWS;
    const bool fuse7 = !e->pair && sk && l7.has_bn && !c.feature_norm;
    float* dz7_fused = nullptr;
    if (e->pair) {      // pairwise heads: no head weight gradient; d out straight from the mined pair matrix (tdnn7 below runs unfused)
        XV_REQUIRE(!e->pair_e2e, "engine_backward: the last loss was the end-to-end validation loss, which has no backward");
        rc = xv_pair_loss_backward(s, &e->pair_cfg, e->out, b, e->Lout, e->Lout, e->labels_dev, e->pair_ws, e->pair_ws_bytes, e->d_small0, e->Lout);
        if (rc) return rc;
    } else if (sk) {
        XvSkinny g = xve_skinny(e, e->dlogits, e->ldl, e->wn, e->ldl, b, e->Lout, e->ldl);
        g.row_coef = e->dnorm; g.row_norm = e->xnorm; g.X = e->out; g.ldx = e->Lout;
        g.C = e->d_small0; g.ldc = e->Lout;
        if (fuse7) {
            dz7_fused = take_dz(e, s);
            XV_REQUIRE_SLOT(dz7_fused);
            skinny_bn_backward(e, g, l7, dz7_fused);
        }
        rc = xv_launch_skinny(s, g);
        if (rc) return rc;
    } else {
        XvGemmNT g = {};
        g.A = e->dlogits; g.lda = e->ldl; g.a_rps = 1; g.a_pitch = 1;
        g.Bt = e->wn; g.ldb = e->ldl;
        g.C = e->d_small0; g.ldc = e->Lout;
        g.M = b; g.N = e->Lout; g.K = e->ldl;
        g.ws = e->ws; g.ws_bytes = e->ws_bytes;
        rc = xv_launch_gemm_nt(s, g);
        if (rc) return rc;
        rc = xv_add_norm_grad(s, e->out, e->dnorm, b, e->Lout, e->d_small0);
        if (rc) return rc;
    }
    if (e->v_ring >= 0) {      // d r of the ring loss was evaluated with the loss (0 when the auxiliary loss was off)
        rc = e->with_margin ? xv_copy_2d(s, gptr(e, e->v_ring), 1, e->scalars + 3, 1, 1, 1) : 0;
        if (!e->with_margin) XV_CHECK_HIP(hipMemsetAsync(gptr(e, e->v_ring), 0, sizeof(float), s));
        if (rc) return rc;
    }
    const float* d = e->d_small0;      // d h7 (not there when tdnn7's BN backward rode on the d-out launch)
    if (c.feature_norm) {
        rc = xv_l2_scaling_backward(s, e->h7, d, b, e->Lout, c.feature_scaling_factor, e->d_small1);
        if (rc) return rc;
        d = e->d_small1;
    }
    if (!sk) {      // tdnn7 -> d a6 (into bufD), tdnn6 -> d pool
        rc = layer_backward(e, s, l7, d, l6.a, b, 1, e->bufD, e->h7);
        if (rc) return rc;
        return layer_backward(e, s, l6, e->bufD, e->pool, b, 1, e->d_small0, nullptr);
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
    float* dz6 = take_dz(e, s);
    XV_REQUIRE_SLOT(dz6);
    XV_REQUIRE(l6.has_bn, "engine_backward: the first segment-level layer has a BatchNorm (tdnn.py:147-163)");
    XvSkinny g = xve_skinny(e, dz7, l7.c_out, vptr(e, l7.v_kernel), l7.c_out, b, l7.c_in, l7.c_out);
    skinny_bn_backward(e, g, l6, dz6);
    rc = xv_launch_skinny(s, g);
    if (rc) return rc;
    rc = layer_wgrad(e, s, l6, e->pool, dz6, b, 1, 0, true);
    if (rc) return rc;
    // d pool = dz6 . W6^T
    g = xve_skinny(e, dz6, l6.c_out, vptr(e, l6.v_kernel), l6.c_out, b, l6.c_in, l6.c_out);
    g.C = e->d_small0; g.ldc = l6.c_in;
    return xv_launch_skinny(s, g);
}

// Through the attention weights into the key network (pooling.py:134-155): d weights from the pooled statistics, softmax
// backward, then att_key1 (dense [+ tanh]) and att_key0 (dense + bn + relu) down to the key input (bufA)
int backward_attention(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    const int F = e->F, b = e->B, Tp = e->Tl[F];
    XvAffine &k0 = e->L[e->K0()], &k1 = e->L[e->K1()];
    const int rows = b * Tp;
    const float scale = c.att_use_scale ? 1.0f / sqrtf((float)k1.c_out) : 1.0f;
    int rc;
    {
        ActScope actv(e, e->L[F - 1]);
        rc = xv_att_pool_backward_weights(s, e->L[F - 1].z, b, Tp, e->P, e->L[F - 1].scale, e->L[F - 1].shift, 1, e->pool, e->d_small0, e->att_dw);
    }
    if (rc) return rc;
    rc = xv_softmax_segments_backward(s, e->att_w, e->att_dw, b, Tp, e->att_ds);
    if (rc) return rc;
    // dzk (fp32) takes the current slot of the fp32 dz ring: a segment-level weight gradient (side stream) may still be
    // reading it.  In split precision its consumer (key1's plane split) runs on `s`, so the slot is not flipped; in
    // fp32 layer_backward() below recognises it as the ring's buffer (dz == Z) and flips the ring itself
    float* dzk = take_dz(e, s);
    XV_REQUIRE_SLOT(dzk);
    // with a BN+ReLU key layer (type 2) this is d key (act = 0 on its output) and layer_backward does the BN/ReLU part
    rc = xv_att_key_backward(s, k1.has_bn ? k1.a : k1.z, rows, k1.c_out, k1.act, vptr(e, e->v_query), scale, e->att_ds, dzk,
                             gptr(e, e->v_query), nullptr, e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = layer_backward(e, s, k1, dzk, k0.a, rows, 1, e->bufD, nullptr);      // -> d att_key0_relu (bufD)
    if (rc) return rc;
    return layer_backward(e, s, k0, e->bufD, e->L[F - 2].a, rows, 1, e->bufA, nullptr);  // -> d (key input) through the keys (bufA)
}

// ghost_vlad backward (stage 1): d pool -> d R through the normalisations; the centres; one pass over x for d A and the value path of
// d x; the softmax; W's bias / weight / data gradients on the column-sum and GEMM launchers; the two paths into x joined in bufD
int backward_vlad(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    XvAffine& a = e->L[e->F - 1];
    const int b = e->B, Tp = e->Tl[e->F], rows = b * Tp, P = e->P, K = e->VK, KG = e->VKG, KGp = e->VKGp;
    const float* cen = vptr(e, e->v_vlad_c);
    int rc = xv_vlad_normalize_backward(s, e->vl_R, e->d_small0, b, K, P, c.vlad_final_l2_norm, e->vl_dR);
    if (rc) return rc;
    rc = xv_vlad_centers_backward(s, e->vl_n, e->vl_dR, cen, b, K, KG, P, c.weight_l2_regularizer, gptr(e, e->v_vlad_c));
    if (rc) return rc;
    rc = xv_vlad_pool_backward(s, a.a, e->vl_A, cen, e->vl_dR, b, Tp, P, K, KG, e->vl_dA, e->vl_dxv);
    if (rc) return rc;
    rc = xv_vlad_softmax_backward(s, e->vl_A, e->vl_dA, rows, KG, KGp, e->vl_dl);
    if (rc) return rc;
    rc = xv_colsum(s, e->vl_dl, rows, KG, KGp, gptr(e, e->v_vlad_b), e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xv_affine_wgrad_ld(s, a.a, rows, 1, P, 1, P, e->vl_dl, KGp, 1, 0, KGp, e->vl_wp, c.weight_l2_regularizer, e->vl_dwp, e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xv_vlad_repitch(s, e->vl_dwp, P, KG, KGp, gptr(e, e->v_vlad_w), KG);
    if (rc) return rc;
    rc = xv_affine_dgrad_ld(s, e->vl_dl, KGp, rows, 1, KGp, 1, e->vl_wp, e->bufD, P, e->ws, e->ws_bytes);
    if (rc) return rc;
    return xv_add_inplace(s, e->bufD, e->vl_dxv, (size_t)rows * P);
}

// backward of frame layer i: a context layer sees chunks of Tl[i] frames, a dense layer one "chunk" per frame
int frame_backward(xv_engine* e, hipStream_t s, int i, const float* da) {
    XvAffine& a = e->L[i];
    const float* x = i > 0 ? e->L[i - 1].a : e->xpad;
    float* dx = i > 0 ? e->bufD : nullptr;
    if (a.k > 1) return layer_backward(e, s, a, da, x, e->B, e->Tl[i], dx, nullptr);
    return layer_backward(e, s, a, da, x, e->B * e->Tl[i + 1], 1, dx, nullptr);
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
    XV_REQUIRE(e->training && e->labels_dev, "engine_backward: needs a training forward + loss_forward first");
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
        if (e->att) { rc = backward_attention(e, s); if (rc) return rc; }
        if (e->vlad) { rc = backward_vlad(e, s); if (rc) return rc; }
        rc = frame_backward(e, s, F - 1, e->vlad ? e->bufD : nullptr);                 // last frame layer (da = pooling backward, materialised for ghost_vlad)
        if (rc) return rc;
        if (e->att) rc = xv_add_inplace(s, e->bufD, e->bufA, (size_t)e->B * e->Tl[F] * e->L[F - 2].c_out);   // the two paths into the key input
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
