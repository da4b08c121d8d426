// Engine, the loss head (XvHead, e->head_): none (a predict-only engine), the softmax family (softmax, asoftmax, additive margin, additive
// angular margin, with the ring / MHE auxiliary losses; loss.py:9-357, xv_loss.hip) and the pairwise heads (semi-hard / angular triplet and
// the end-to-end validation loss; loss.py:358-705, xv_triplet.hip) and the GE2E training loss with its two trainable scalars (loss.py:903-982,
// xv_triplet.hip), one function per phase of the engine's life - configuration, variables,
// arena, workspace, weight preparation, loss forward, weight gradient, d out, ring gradient, regularisation, endpoints.  The only engine
// unit that reads the loss kind: a new head is a new case in each function here.
#include <algorithm>

#include "xv_engine.h"

namespace {
bool is_softmax(const xv_engine* e) { return e->head_.kind == XV_HEAD_SOFTMAX; }
bool is_pair(const xv_engine* e) { return e->head_.kind == XV_HEAD_PAIR; }
bool is_ge2e(const xv_engine* e) { return e->head_.kind == XV_HEAD_GE2E; }
}  // namespace

int xvh_check_config(const xv_config* cfg) {
    XV_REQUIRE(cfg->loss_kind >= XV_LOSS_SOFTMAX && cfg->loss_kind <= XV_LOSS_GE2E, "Not implement loss kind %d", cfg->loss_kind);
    if (cfg->loss_kind == XV_LOSS_ASOFTMAX && cfg->num_speakers > 0)
        XV_REQUIRE(cfg->margin_m == 1.f || cfg->margin_m == 2.f || cfg->margin_m == 4.f, "[ERROR] m=%d is not unsupported.", (int)cfg->margin_m);
    XV_REQUIRE(!cfg->aux_mhe || cfg->num_speakers == 0 || cfg->loss_kind != XV_LOSS_SOFTMAX,
               "engine_create: mhe_loss needs a loss with normalised speaker weights (asoftmax / additive margin losses)");
    return 0;
}

void xvh_configure(xv_engine* e) {
    xv_config& c = e->cfg;
    XvHead& h = e->head_;
    // no ring / MHE term, and the variable softmax_ringloss/r is never created:
    //  - asoftmax with m = 1 returns its plain cross entropy before aux_loss_func is reached (loss.py:110-115)
    //  - the reference's triplet functions never call aux_loss_func (loss.py:358-634), nor does its GE2E loss (loss.py:903-982)
    if ((c.loss_kind == XV_LOSS_ASOFTMAX && c.margin_m == 1.f) || c.loss_kind >= XV_LOSS_SEMIHARD_TRIPLET) c.aux_ring = c.aux_mhe = 0;
    const bool pair = c.loss_kind == XV_LOSS_SEMIHARD_TRIPLET || c.loss_kind == XV_LOSS_ANGULAR_TRIPLET;
    const bool ge2e = c.loss_kind == XV_LOSS_GE2E;
    h.N = pair || ge2e ? 0 : c.num_speakers;      // pairwise heads and GE2E: no softmax/output variables
    h.kind = pair ? XV_HEAD_PAIR : (ge2e ? XV_HEAD_GE2E : (h.N > 0 ? XV_HEAD_SOFTMAX : XV_HEAD_NONE));
    h.ldl = h.N > 0 ? (int)xv_align(h.N, 4) : 0;
}

extern "C" int xv_engine_set_pair_loss(xv_engine* e, const xv_pair_loss_config* cfg) {
    XV_REQUIRE(e && cfg, "engine_set_pair_loss: null argument");
    XV_REQUIRE(is_pair(e), "engine_set_pair_loss: the engine's loss_kind %d is not a pairwise head (semihard_triplet_loss 4, angular_triplet_loss 5)", e->cfg.loss_kind);
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_pair_loss_config), "engine_set_pair_loss: xv_pair_loss_config.struct_bytes is %d, this library's struct has %zu bytes",
               cfg->struct_bytes, sizeof(xv_pair_loss_config));
    XV_REQUIRE(cfg->kind == (e->cfg.loss_kind == XV_LOSS_SEMIHARD_TRIPLET ? XV_PAIR_SEMIHARD : XV_PAIR_ANGULAR),
               "engine_set_pair_loss: pair loss kind %d does not belong to the engine's loss_kind %d", cfg->kind, e->cfg.loss_kind);
    XV_REQUIRE(cfg->valid_speakers >= 0 && cfg->valid_segments >= 0, "engine_set_pair_loss: negative validation layout %d x %d", cfg->valid_speakers, cfg->valid_segments);
    e->head_.pair_cfg = *cfg;
    e->head_.pair_set = true;
    return 0;
}

extern "C" int xv_engine_set_ge2e_loss(xv_engine* e, const xv_ge2e_config* cfg) {
    XV_REQUIRE(e && cfg, "engine_set_ge2e_loss: null argument");
    XV_REQUIRE(is_ge2e(e), "engine_set_ge2e_loss: the engine's loss_kind %d is not ge2e_loss (6)", e->cfg.loss_kind);
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_ge2e_config), "engine_set_ge2e_loss: xv_ge2e_config.struct_bytes is %d, this library's struct has %zu bytes",
               cfg->struct_bytes, sizeof(xv_ge2e_config));
    XV_REQUIRE(cfg->loss_type == XV_GE2E_SOFTMAX || cfg->loss_type == XV_GE2E_CONTRASTIVE,
               "engine_set_ge2e_loss: The GE2E only support softmax and contrastive loss (loss_type %d)", cfg->loss_type);
    XV_REQUIRE(cfg->speakers >= 1 && cfg->segments >= 1, "engine_set_ge2e_loss: %d speakers x %d segments", cfg->speakers, cfg->segments);
    XV_REQUIRE(cfg->segments != 1, "engine_set_ge2e_loss: num_segments_per_speaker is 1: a row needs another row of its speaker (assert num_segments_per_speaker != 1)");
    XV_REQUIRE((long)cfg->speakers * cfg->segments <= 1024, "engine_set_ge2e_loss: %d speakers x %d segments, 1 .. 1024 rows are supported", cfg->speakers,
               cfg->segments);
    XV_REQUIRE(cfg->valid_speakers >= 0 && cfg->valid_segments >= 0, "engine_set_ge2e_loss: negative validation layout %d x %d", cfg->valid_speakers, cfg->valid_segments);
    e->head_.ge2e_cfg = *cfg;
    e->head_.ge2e_set = true;
    return 0;
}

void xvh_declare_variables(xv_engine* e) {
    XvHead& h = e->head_;
    if (is_ge2e(e)) {      // scalars (loss.py:923-924), as softmax_ringloss/r is; the host initialiser sets them from init_end2end_w / _b
        h.v_ge2e_w = xve_add_var(e, "ge2e/w", {}, true);
        h.v_ge2e_b = xve_add_var(e, "ge2e/b", {}, true);
    }
    if (!is_softmax(e)) return;
    h.v_loss_kernel = xve_add_var(e, "softmax/output/kernel", {e->Lout, h.N}, true);
    if (e->cfg.loss_kind == XV_LOSS_SOFTMAX) h.v_loss_bias = xve_add_var(e, "softmax/output/bias", {h.N}, true);
    if (e->cfg.aux_ring) h.v_ring = xve_add_var(e, "softmax_ringloss/r", {}, true);      // scalar, loss.py:1008-1011
}

void xvh_arena(xv_engine* e, const ArenaPlan& p, ArenaCursor& take) {
    XvHead& h = e->head_;
    const size_t B = p.B;
    if (is_softmax(e) && e->cfg.aux_mhe) {
        take(h.mhe_coef, 1 + 2 * (size_t)e->Lout);
        take(h.mhe_counts, h.N);
    }
    if (is_softmax(e)) {
        take(h.logits, B * h.ldl); take(h.dlogits, B * h.ldl);
        take(h.dnorm, B); take(h.row_loss, B);
        take(h.inv_norm, h.N);
        take(h.wn, (size_t)e->Lout * h.ldl);
        take(h.wnt, (size_t)h.N * e->Lout);
        take(h.dwn, (size_t)e->Lout * h.ldl);
    }
    if (is_ge2e(e)) {      // one workspace for the validation loss and for the training loss in every N x M layout of as many rows as the heads take
        const int rows = (int)std::min<size_t>(B, 1024);
        h.pair_ws_bytes = xv_pair_loss_workspace_bytes(rows, e->Lout);
        for (int m = 2; m <= rows; ++m) h.pair_ws_bytes = std::max(h.pair_ws_bytes, xv_ge2e_loss_workspace_bytes(rows / m, m, e->Lout));
        take(h.pair_ws, h.pair_ws_bytes / sizeof(float));
        take(h.pair_stats, 4);
    }
    if (is_pair(e)) {      // G, the pair-matrix gradient and its symmetrised form for as many rows as the heads take (xv_pair_loss_workspace_bytes)
        h.pair_ws_bytes = xv_pair_loss_workspace_bytes((int)std::min<size_t>(B, 1024), e->Lout);
        take(h.pair_ws, h.pair_ws_bytes / sizeof(float));
        take(h.pair_stats, 4);
    }
}

void xvh_arena_tail(xv_engine* e, const ArenaPlan& p, ArenaCursor& take) { take(e->head_.xnorm, p.B); }

size_t xvh_workspace_bytes(const xv_engine* e, const ArenaPlan& p) {
    if (!is_softmax(e)) return 0;
    const XvHead& h = e->head_;
    return std::max((size_t)xv_tn_splits_direct(e->Lout, h.ldl, (int)p.B) * e->Lout * h.ldl * sizeof(float), (size_t)16 * p.B * h.ldl * sizeof(float));
}

int xvh_prep_weights(xv_engine* e, hipStream_t s) {
    if (!is_softmax(e)) return 0;
    XvHead& h = e->head_;
    return xv_loss_prep_weight(s, vptr(e, h.v_loss_kernel), e->Lout, h.N, e->cfg.loss_kind != XV_LOSS_SOFTMAX, h.inv_norm, h.wn, h.ldl, h.wnt);
}

namespace {

// pairwise heads: no logits, no head weights; the embedding is the whole input
int pair_loss_forward(xv_engine* e, hipStream_t s, const int32_t* labels) {
    const xv_config& c = e->cfg;
    XvHead& h = e->head_;
    const int b = e->B;
    XV_REQUIRE(h.pair_set, "engine_loss_forward: loss_kind %d (%s) needs its options: call xv_engine_set_pair_loss first", c.loss_kind,
               c.loss_kind == XV_LOSS_SEMIHARD_TRIPLET ? "semihard_triplet_loss" : "angular_triplet_loss");
    h.pair_e2e = !h.with_margin && c.loss_kind == XV_LOSS_ANGULAR_TRIPLET;      // trainer.py:272-275; the semi-hard loss validates as it trains
    e->reg_valid = false;
    if (h.pair_e2e) {
        XV_REQUIRE((long)h.pair_cfg.valid_speakers * h.pair_cfg.valid_segments == b,
                   "engine_loss_forward: the end-to-end validation loss takes num_valid_speakers_per_batch x num_valid_segments_per_speaker = %d x %d rows, the batch has %d",
                   h.pair_cfg.valid_speakers, h.pair_cfg.valid_segments, b);
        return xv_e2e_valid_loss(s, e->out, h.pair_cfg.valid_speakers, h.pair_cfg.valid_segments, e->Lout, e->Lout, e->scalars + 0, h.pair_ws, h.pair_ws_bytes);
    }
    return xv_pair_loss_forward(s, &h.pair_cfg, e->out, b, e->Lout, e->Lout, labels, e->scalars + 0, h.pair_stats, h.pair_ws, h.pair_ws_bytes);
}

// GE2E: the training loss on speakers x segments rows with the scalars ge2e/w and ge2e/b; validation as the angular kind's
int ge2e_loss_forward(xv_engine* e, hipStream_t s) {
    XvHead& h = e->head_;
    const int b = e->B;
    XV_REQUIRE(h.ge2e_set, "engine_loss_forward: loss_kind %d (ge2e_loss) needs its options: call xv_engine_set_ge2e_loss first", e->cfg.loss_kind);
    h.pair_e2e = !h.with_margin;      // trainer.py:272-275
    e->reg_valid = false;
    if (h.pair_e2e) {
        XV_REQUIRE((long)h.ge2e_cfg.valid_speakers * h.ge2e_cfg.valid_segments == b,
                   "engine_loss_forward: the end-to-end validation loss takes num_valid_speakers_per_batch x num_valid_segments_per_speaker = %d x %d rows, the batch has %d",
                   h.ge2e_cfg.valid_speakers, h.ge2e_cfg.valid_segments, b);
        return xv_e2e_valid_loss(s, e->out, h.ge2e_cfg.valid_speakers, h.ge2e_cfg.valid_segments, e->Lout, e->Lout, e->scalars + 0, h.pair_ws, h.pair_ws_bytes);
    }
    XV_REQUIRE((long)h.ge2e_cfg.speakers * h.ge2e_cfg.segments == b,
               "engine_loss_forward: ge2e_loss takes num_speakers_per_batch x num_segments_per_speaker = %d x %d rows, the batch has %d", h.ge2e_cfg.speakers,
               h.ge2e_cfg.segments, b);
    return xv_ge2e_loss_forward(s, &h.ge2e_cfg, e->out, e->Lout, e->Lout, vptr(e, h.v_ge2e_w), vptr(e, h.v_ge2e_b), e->scalars + 0, h.pair_stats, h.pair_ws,
                                h.pair_ws_bytes);
}

// the softmax family: logits on the normalised (or plain) speaker weights, the margin rows, the auxiliary losses
int softmax_loss_forward(xv_engine* e, hipStream_t s, const int32_t* labels, int global_step) {
    const xv_config& c = e->cfg;
    XvHead& h = e->head_;
    const int b = e->B;
    int rc;
    const float* bias = h.v_loss_bias >= 0 ? vptr(e, h.v_loss_bias) : nullptr;
    if (e->sk && b <= XV_SEGMENT_MAX_ROWS) {
        XvSkinny g = xve_skinny(e, e->out, e->Lout, h.wnt, e->Lout, b, h.N, e->Lout);
        g.bias = bias; g.C = h.logits; g.ldc = h.ldl;
        rc = xv_launch_skinny(s, g);
    } else {
        XvGemmNT g = {};
        g.A = e->out; g.lda = e->Lout; g.a_rps = 1; g.a_pitch = 1;
        g.Bt = h.wnt; g.ldb = e->Lout;
        g.C = h.logits; g.ldc = h.ldl;
        g.M = b; g.N = h.N; g.K = e->Lout;
        g.bias = bias;
        g.ws = e->ws; g.ws_bytes = e->ws_bytes;
        rc = xv_launch_gemm_nt(s, g);
    }
    if (rc) return rc;
    // lambda schedule, loss.py:144-145 (host side: global_step is a fed placeholder, trainer.py:507)
    double lam = (double)c.lambda_base * pow(1.0 + (double)c.lambda_gamma * (double)global_step, -(double)c.lambda_power);
    if (lam < (double)c.lambda_min) lam = (double)c.lambda_min;
    h.lambda = (float)lam;
    int kind = c.loss_kind;
    float m = c.margin_m;
    if (!h.with_margin && kind != XV_LOSS_SOFTMAX) { kind = XV_LOSS_ASOFTMAX; m = 1.0f; }   // trainer.py:261-271
    // one launch: the rows, ||out[r]|| (divides the ||x|| gradient in backward) and the mean (last ticket of sk_tickets)
    rc = xv_margin_softmax_rows_ex(s, kind, h.logits, b, h.N, h.ldl, e->out, e->Lout, labels, m, h.lambda, h.dlogits, h.dnorm,
                                   h.row_loss, e->scalars + 0, h.xnorm, e->sk_tickets + (e->sk_ntickets - 1));
    if (rc) return rc;
    // auxiliary losses are part of the training loss only (trainer.py:279-289 clears aux_loss_func for validation)
    if (h.with_margin && c.aux_ring) {
        rc = xv_ring_loss(s, e->out, b, e->Lout, e->Lout, vptr(e, h.v_ring), c.ring_loss_lambda, e->scalars + 0, h.dnorm, e->scalars + 3);
        if (rc) return rc;
    }
    if (h.with_margin && c.aux_mhe) {
        rc = xv_mhe_loss(s, h.wn, e->Lout, h.N, h.ldl, labels, b, c.mhe_lambda, e->scalars + 0, h.mhe_coef, h.mhe_counts);
        if (rc) return rc;
    }
    e->reg_valid = false;
    return 0;
}

}  // namespace

int xvh_loss_forward(xv_engine* e, hipStream_t s, const int32_t* labels, int global_step) {
    if (is_ge2e(e)) return ge2e_loss_forward(e, s);      // (labels are not read, as in the reference)
    return is_pair(e) ? pair_loss_forward(e, s, labels) : softmax_loss_forward(e, s, labels, global_step);
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
// (pairwise heads: no head weights, nothing to do)
int xvh_wgrad(xv_engine* e, hipStream_t s) {
    if (!is_softmax(e)) return 0;
    const xv_config& c = e->cfg;
    XvHead& h = e->head_;
    const int b = e->B;
    int rc = 0;
    hipStream_t ss = e->concurrent ? e->side2 : s;
    void* lws = e->concurrent ? e->ws_side2 : e->ws_side;
    if (e->concurrent) {
        rc = xve_chain(s, ss, e->ev_dz);
        if (rc) return rc;
    }
    XvGemmTN w = {};
    w.A = e->out; w.lda = e->Lout; w.a_rps = b; w.a_pitch = b;
    w.B = h.dlogits; w.ldb = h.ldl; w.b_rps = b; w.b_pitch = b;
    w.M = e->Lout; w.N = h.ldl; w.R = b;
    w.direct = 1;
    w.splits = xv_tn_splits_direct(w.M, w.N, w.R);
    XV_REQUIRE(w.splits == 1 || (size_t)w.splits * w.M * w.N * sizeof(float) <= e->ws_bytes, "engine_backward: workspace too small for the loss weight gradient");
    // unsplit (xv_tn_plan: a short reduction over many tiles): the one "slab" IS d wn [Lout][ldl] - no slab sum
    w.P = w.splits == 1 ? h.dwn : (float*)lws;
    rc = xv_launch_gemm_tn(ss, w);
    if (rc) return rc;
    if (w.splits > 1) {
        rc = xv_launch_wgrad_reduce(ss, w.P, w.splits, 1, e->Lout, e->Lout, h.ldl, h.ldl, nullptr, 0, 0.f, h.dwn, h.ldl);
        if (rc) return rc;
    }
    if (h.with_margin && c.aux_mhe) {
        rc = xv_mhe_add_grad(ss, h.dwn, e->Lout, h.N, h.ldl, h.mhe_coef, h.mhe_counts);
        if (rc) return rc;
    }
    rc = xv_loss_weight_backward(ss, h.dwn, h.ldl, h.wn, h.ldl, h.inv_norm, vptr(e, h.v_loss_kernel), e->Lout, h.N,
                                 c.loss_kind != XV_LOSS_SOFTMAX, xve_output_l2(c), gptr(e, h.v_loss_kernel), lws, e->ws_bytes);
    if (rc) return rc;
    if (h.v_loss_bias >= 0) {
        rc = xv_colsum(ss, h.dlogits, b, h.N, h.ldl, gptr(e, h.v_loss_bias), lws, e->ws_bytes);
        if (rc) return rc;
    }
    if (e->concurrent) {
        XV_CHECK_HIP(hipEventRecord(e->ev_lw, ss));
        e->lw_pending = true;
    }
    return 0;
}

int xvh_dout(xv_engine* e, hipStream_t s, bool sk, float** dz7_fused) {
    XvHead& h = e->head_;
    const int b = e->B;
    *dz7_fused = nullptr;
    if (is_ge2e(e)) {      // d out, d w and d b from the forward's workspace (tdnn7 then runs unfused, as behind the pairwise heads)
        XV_REQUIRE(!h.pair_e2e, "engine_backward: the last loss was the end-to-end validation loss, which has no backward");
        return xv_ge2e_loss_backward(s, &h.ge2e_cfg, e->out, e->Lout, e->Lout, vptr(e, h.v_ge2e_w), vptr(e, h.v_ge2e_b), h.pair_ws, h.pair_ws_bytes, e->d_small0,
                                     e->Lout, gptr(e, h.v_ge2e_w), gptr(e, h.v_ge2e_b));
    }
    if (is_pair(e)) {      // pairwise heads: no head weight gradient; d out straight from the mined pair matrix (tdnn7 then runs unfused)
        XV_REQUIRE(!h.pair_e2e, "engine_backward: the last loss was the end-to-end validation loss, which has no backward");
        return xv_pair_loss_backward(s, &h.pair_cfg, e->out, b, e->Lout, e->Lout, h.labels_dev, h.pair_ws, h.pair_ws_bytes, e->d_small0, e->Lout);
    }
    // d out = dlogits . wn^T   (pad column of both is zero, so K = ldl is exact), + the gradient through ||out|| (loss.py:122,147).
    // Fused form (xv_skinny.hip): one launch, and with a BatchNorm in tdnn7 and no l2_scaling in between, tdnn7's BN backward too
    if (sk) {
        XvAffine& l7 = e->L[e->S1()];
        XvSkinny g = xve_skinny(e, h.dlogits, h.ldl, h.wn, h.ldl, b, e->Lout, h.ldl);
        g.row_coef = h.dnorm; g.row_norm = h.xnorm; g.X = e->out; g.ldx = e->Lout;
        g.C = e->d_small0; g.ldc = e->Lout;
        if (l7.has_bn && !e->cfg.feature_norm) {
            *dz7_fused = xve_take_dz(e, s);
            XV_REQUIRE_SLOT(*dz7_fused);
            xve_skinny_bn_backward(e, g, l7, *dz7_fused);
        }
        return xv_launch_skinny(s, g);
    }
    XvGemmNT g = {};
    g.A = h.dlogits; g.lda = h.ldl; g.a_rps = 1; g.a_pitch = 1;
    g.Bt = h.wn; g.ldb = h.ldl;
    g.C = e->d_small0; g.ldc = e->Lout;
    g.M = b; g.N = e->Lout; g.K = h.ldl;
    g.ws = e->ws; g.ws_bytes = e->ws_bytes;
    int rc = xv_launch_gemm_nt(s, g);
    if (rc) return rc;
    return xv_add_norm_grad(s, e->out, h.dnorm, b, e->Lout, e->d_small0);
}

int xvh_ring_grad(xv_engine* e, hipStream_t s) {
    XvHead& h = e->head_;
    if (h.v_ring < 0) return 0;
    // d r of the ring loss was evaluated with the loss (0 when the auxiliary loss was off)
    int rc = h.with_margin ? xv_copy_2d(s, gptr(e, h.v_ring), 1, e->scalars + 3, 1, 1, 1) : 0;
    if (!h.with_margin) XV_CHECK_HIP(hipMemsetAsync(gptr(e, h.v_ring), 0, sizeof(float), s));
    return rc;
}

int xvh_reg_loss(xv_engine* e, hipStream_t s) {
    if (!is_softmax(e)) return 0;
    const int v = e->head_.v_loss_kernel;
    return xv_sumsq_ordered(s, vptr(e, v), e->vars[v].count, 0.5f * xve_output_l2(e->cfg), e->scalars + 1, (float*)e->ws);
}

int xvh_endpoint(xv_engine* e, const std::string& n, const XvView& v) {
    if (n == "logits" && is_softmax(e)) return v.set(e->head_.logits, e->B, e->head_.N, e->head_.ldl);
    return XV_EP_UNKNOWN;
}
