// Engine, the pooling layer (XvPooling, e->pool_): statistics pooling (pooling.py:9-45), single-head self-attention on a key network
// (pooling.py:48-192) and ghost_vlad (pooling.py:195-277), one function per phase of the engine's life - configuration, variables, key layers,
// arena, workspace, forward, backward, regularisation, endpoints.  The only engine unit that reads the pooling kind: a new kind is a new
// case in each function here (and, for questions the layer code asks, in XvPooling itself, xv_engine.h).
#include <algorithm>

#include "xv_engine.h"

namespace {
bool is_att(const xv_engine* e) { return e->pool_.kind == XV_POOL_SELF_ATTENTION; }
bool is_vlad(const xv_engine* e) { return e->pool_.kind == XV_POOL_GHOST_VLAD; }
}  // namespace

int xvp_check_config(const xv_config* cfg) {
    XV_REQUIRE(cfg->pooling == XV_POOL_STATISTICS || cfg->pooling == XV_POOL_SELF_ATTENTION || cfg->pooling == XV_POOL_GHOST_VLAD,
               "Not implement pooling kind %d", cfg->pooling);
    if (cfg->pooling == XV_POOL_GHOST_VLAD) {
        XV_REQUIRE(cfg->precision == XV_PRECISION_F32, "engine_create: ghost_vlad pooling runs in precision f32 only (not f16x3)");
        XV_REQUIRE(cfg->vlad_num_centers >= 1 && cfg->vlad_num_ghosts >= 0 && cfg->vlad_num_centers + cfg->vlad_num_ghosts <= 64,
                   "engine_create: ghost_vlad needs vlad_num_centers >= 1, vlad_num_ghosts >= 0 and at most 64 clusters in all (got %d + %d)",
                   cfg->vlad_num_centers, cfg->vlad_num_ghosts);
    }
    if (cfg->pooling == XV_POOL_SELF_ATTENTION) {
        XV_REQUIRE(cfg->att_key0_nodes > 0 && cfg->att_key0_nodes % 4 == 0 && cfg->att_key1_nodes > 0 && cfg->att_key1_nodes % 4 == 0,
                   "engine_create: att_key_num_nodes must be two positive multiples of 4 (got %d, %d)", cfg->att_key0_nodes, cfg->att_key1_nodes);
        XV_REQUIRE(cfg->att_key_type >= 0 && cfg->att_key_type <= 3, "engine_create: att_key_network_type %d is not one of 0..3", cfg->att_key_type);
    }
    XV_REQUIRE(!(cfg->relu_type != XV_RELU_RELU && cfg->pooling == XV_POOL_SELF_ATTENTION && cfg->att_key_type == 1),
               "engine_create: att_key_network_type 1 (affine + relu inside the score kernel) is built for a plain ReLU; use type 0, 2 or 3 with prelu / lrelu");
    return 0;
}

void xvp_configure(xv_engine* e) {
    const xv_config& c = e->cfg;
    XvPooling& p = e->pool_;
    p.kind = c.pooling;
    p.P = c.num_nodes_pooling_layer;
    p.VK = is_vlad(e) ? c.vlad_num_centers : 0; p.VG = is_vlad(e) ? c.vlad_num_ghosts : 0;
    p.VKG = p.VK + p.VG; p.VKGp = (int)xv_align(p.VKG, 4);
    p.pool_dim = is_vlad(e) ? p.VK * p.P : 2 * p.P;
}

void xvp_key_layers(const xv_engine* e, int c_key, std::vector<XvLayerSpec>& specs) {
    if (!is_att(e)) return;
    const xv_config& c = e->cfg;
    const int F = e->F;
    // self-attention key network (pooling.py:78-96): dense+bn+relu on the key input, then dense (+tanh)
    specs.push_back({"att_key0", "dense", "attention/att_key0/", 1, c_key, c.att_key0_nodes, true, true, false, F - 2, 0});
    // last key layer (att_key_network_type): 0 affine, 1 + relu, 3 + tanh as an activation inside the score kernels; 2 = + bn + relu
    specs.push_back({"att_key1", "dense", "attention/att_key1/", 1, c.att_key0_nodes, c.att_key1_nodes, c.att_key_type == 2, c.att_key_type == 2, false,
                     F + 2, c.att_key_type == 2 ? 0 : c.att_key_type});
}

void xvp_declare_variables(xv_engine* e) {
    XvPooling& p = e->pool_;
    if (is_att(e)) p.v_query = xve_add_var(e, "tdnn/attention/query", {1, e->L[e->K1()].c_out}, true);   // [heads, key dim], pooling.py:131
    if (is_vlad(e)) {      // pooling.py:242-256: the variables of the "vlad" scope sit where the attention variables sit
        p.v_vlad_w = xve_add_var(e, "tdnn/vlad/vlad_weight_affine/kernel", {p.P, p.VKG}, true);
        p.v_vlad_b = xve_add_var(e, "tdnn/vlad/vlad_weight_affine/bias", {p.VKG}, true);
        p.v_vlad_c = xve_add_var(e, "tdnn/vlad/vlad_centers", {p.VKG, p.P}, true);
    }
}

void xvp_arena(xv_engine* e, const ArenaPlan& pl, ArenaCursor& take) {
    XvPooling& p = e->pool_;
    const size_t B = pl.B, rows_pool = pl.rows[e->F];
    if (is_att(e)) {
        take(p.att_score, rows_pool); take(p.att_w, rows_pool); take(p.att_dw, rows_pool); take(p.att_ds, rows_pool);
        take(p.bufA, rows_pool * e->L[e->F - 2].c_out);
    }
    if (is_vlad(e)) {
        const size_t kgp = p.VKGp, kg = p.VKG;
        take(p.vl_wp, (size_t)p.P * kgp); take(p.vl_wt, kgp * p.P); take(p.vl_bp, kgp); take(p.vl_dwp, (size_t)p.P * kgp);
        take(p.vl_logits, rows_pool * kgp); take(p.vl_dl, rows_pool * kgp);
        take(p.vl_A, rows_pool * kg); take(p.vl_dA, rows_pool * kg);
        take(p.vl_R, B * p.pool_dim); take(p.vl_dR, B * p.pool_dim); take(p.vl_n, B * (size_t)p.VK);
        if (e->has_loss()) take(p.vl_dxv, rows_pool * p.P);      // (backward only: a predict-only engine does not pay for it)
    }
    take(p.pool, B * (size_t)p.pool_dim);
}

void xvp_arena_tail(xv_engine* e, const ArenaPlan& pl, ArenaCursor& take) {
    take(e->pool_.pool_wpos, pl.B * (size_t)e->pool_.P);
    take(e->pool_.pool_amax, pl.B * (size_t)e->pool_.P);
}

size_t xvp_workspace_bytes(const xv_engine* e, const ArenaPlan& pl) {
    const XvPooling& p = e->pool_;
    const size_t rows_pool = pl.rows[e->F];
    size_t ws = xv_op_workspace_bytes((int)pl.rows[1], 2 * p.P, 2 * p.P);
    if (is_vlad(e))       // the assignment layer's weight gradient [P][KGp] over the pooled rows
        ws = std::max(ws, (size_t)xv_tn_splits(p.P, p.VKGp, (int)rows_pool) * p.P * p.VKGp * sizeof(float));
    if (is_att(e)) {      // xv_att_key_backward: per-chunk partials + the column-sum workspace
        const int k1 = e->cfg.att_key1_nodes;
        ws = std::max(ws, 2 * ((size_t)xv_cdiv(rows_pool, 64) * 2 * k1 * sizeof(float) + xv_op_workspace_bytes((int)rows_pool, k1, k1)) + 4096);
    }
    return ws;
}

namespace {

// ghost_vlad (pooling.py:225-277) on the last frame layer's ReLU output: the assignment logits on the dense GEMM (W and the bias as
// copies padded to whole column quads), softmax over the K + G clusters, the residual sums of the K centres, the normalisations
int vlad_forward(xv_engine* e, hipStream_t s, int b, int Tp, const int32_t* frames, int shrink) {
    const xv_config& c = e->cfg;
    XvPooling& p = e->pool_;
    XvAffine& a = e->L[e->F - 1];
    const int rows = b * Tp, P = p.P, K = p.VK, KG = p.VKG, KGp = p.VKGp;
    int rc = xv_vlad_repitch(s, vptr(e, p.v_vlad_w), P, KG, KG, p.vl_wp, KGp);
    if (rc) return rc;
    rc = xv_vlad_repitch(s, vptr(e, p.v_vlad_b), 1, KG, KG, p.vl_bp, KGp);
    if (rc) return rc;
    rc = xv_prep_weight_fwd(s, p.vl_wp, 1, P, KGp, p.vl_wt, P);
    if (rc) return rc;
    rc = xv_affine_forward(s, a.a, rows, 1, P, 1, p.vl_wt, p.vl_bp, p.vl_logits, KGp, KGp, nullptr, e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xv_vlad_softmax(s, p.vl_logits, rows, KG, KGp, p.vl_A);
    if (rc) return rc;
    rc = xv_vlad_pool_forward_ex(s, a.a, p.vl_A, vptr(e, p.v_vlad_c), b, Tp, P, K, KG, frames, shrink, p.vl_R, p.vl_n);
    if (rc) return rc;
    return xv_vlad_normalize_forward(s, p.vl_R, b, K, P, c.vlad_final_l2_norm, p.pool);
}

// The attention weights of the pooled frames: the key network on the last-but-one frame layer's output, scores, softmax
int attention_forward(xv_engine* e, hipStream_t s, int b, int Tp, const int32_t* frames, int shrink) {
    XvPooling& p = e->pool_;
    // key network on the last-but-one frame layer's output (tdnn4_relu; in split precision its planes are still there):
    // att_key0 = dense+bn+relu, att_key1 = dense (+ bn + relu: att_key_network_type 2, kept in fp32 for the score)
    int rc = xve_layer_forward(e, s, e->K0(), b * Tp, 1);
    if (rc) return rc;
    rc = xve_layer_forward(e, s, e->K1(), b * Tp, 1);
    if (rc) return rc;
    // scores = key.query (/ sqrt(dk)), weights = softmax over the frames of each chunk (pooling.py:134-148)
    XvAffine& k1 = e->L[e->K1()];
    const float scale = e->cfg.att_use_scale ? 1.0f / sqrtf((float)k1.c_out) : 1.0f;
    rc = xv_att_score(s, k1.has_bn ? k1.a : k1.z, b * Tp, k1.c_out, k1.c_out, k1.act, vptr(e, p.v_query), scale, p.att_score);
    if (rc) return rc;
    return xv_softmax_segments_ex(s, p.att_score, b, Tp, p.att_w, frames, shrink);
}

}  // namespace

int xvp_forward(xv_engine* e, hipStream_t s, int b, int t, const int32_t* frames) {
    XvPooling& p = e->pool_;
    const int Tp = e->Tl[e->F];      // pooled frames
    if (is_vlad(e)) return vlad_forward(e, s, b, Tp, frames, t - Tp);
    if (is_att(e)) {
        const int rc = attention_forward(e, s, b, Tp, frames, t - Tp);
        if (rc) return rc;
    }
    // the last frame layer's BN + ReLU is applied inside the pooling reduction: its [b*t][1500] activation is never written
    XvAffine& a = e->L[e->F - 1];
    ActScope act(e, a);
    return xv_stat_pool_forward_bn_ex(s, a.z, b, Tp, p.P, a.scale, a.shift, 1, is_att(e) ? p.att_w : nullptr, p.pool, e->training ? p.pool_wpos : nullptr,
                                      e->f16 ? p.pool_amax : nullptr /* bounds |d a| for the dz planes' scale */, frames, t - Tp, a.ldz);
}

// The upstream gradient of the last frame layer (tdnn5): the (attention-weighted) statistics-pooling backward of (pool, d pool)
XvBnUpstream xvp_upstream(const xv_engine* e) {
    const XvPooling& p = e->pool_;
    XvBnUpstream up = {};
    up.pool_out = p.pool; up.dpool = e->d_small0; up.pool_t = e->Tl[e->F]; up.weights = is_att(e) ? p.att_w : nullptr;
    if (p.pool_closed_form) { up.wpos = p.pool_wpos; up.pamax = p.pool_amax; }
    return up;
}

namespace {

// Through the attention weights into the key network (pooling.py:134-155): d weights from the pooled statistics, softmax
// backward, then att_key1 (dense [+ tanh]) and att_key0 (dense + bn + relu) down to the key input (bufA)
int backward_attention(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    XvPooling& p = e->pool_;
    const int F = e->F, b = e->B, Tp = e->Tl[F];
    XvAffine &k0 = e->L[e->K0()], &k1 = e->L[e->K1()];
    const int rows = b * Tp;
    const float scale = c.att_use_scale ? 1.0f / sqrtf((float)k1.c_out) : 1.0f;
    int rc;
    {
        ActScope actv(e, e->L[F - 1]);
        rc = xv_att_pool_backward_weights(s, e->L[F - 1].z, b, Tp, p.P, e->L[F - 1].scale, e->L[F - 1].shift, 1, p.pool, e->d_small0, p.att_dw);
    }
    if (rc) return rc;
    rc = xv_softmax_segments_backward(s, p.att_w, p.att_dw, b, Tp, p.att_ds);
    if (rc) return rc;
    // dzk (fp32) takes the current slot of the fp32 dz ring: a segment-level weight gradient (side stream) may still be
    // reading it.  In split precision its consumer (key1's plane split) runs on `s`, so the slot is not flipped; in
    // fp32 xve_layer_backward() below recognises it as the ring's buffer (dz == Z) and flips the ring itself
    float* dzk = xve_take_dz(e, s);
    XV_REQUIRE_SLOT(dzk);
    // with a BN+ReLU key layer (type 2) this is d key (act = 0 on its output) and xve_layer_backward does the BN/ReLU part
    rc = xv_att_key_backward(s, k1.has_bn ? k1.a : k1.z, rows, k1.c_out, k1.act, vptr(e, p.v_query), scale, p.att_ds, dzk,
                             gptr(e, p.v_query), nullptr, e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xve_layer_backward(e, s, k1, dzk, k0.a, rows, 1, e->bufD, nullptr);      // -> d att_key0_relu (bufD)
    if (rc) return rc;
    return xve_layer_backward(e, s, k0, e->bufD, e->L[F - 2].a, rows, 1, p.bufA, nullptr);  // -> d (key input) through the keys (bufA)
}

// ghost_vlad backward (stage 1): d pool -> d R through the normalisations; the centres; one pass over x for d A and the value path of
// d x; the softmax; W's bias / weight / data gradients on the column-sum and GEMM launchers; the two paths into x joined in bufD
int backward_vlad(xv_engine* e, hipStream_t s) {
    const xv_config& c = e->cfg;
    XvPooling& p = e->pool_;
    XvAffine& a = e->L[e->F - 1];
    const int b = e->B, Tp = e->Tl[e->F], rows = b * Tp, P = p.P, K = p.VK, KG = p.VKG, KGp = p.VKGp;
    const float* cen = vptr(e, p.v_vlad_c);
    int rc = xv_vlad_normalize_backward(s, p.vl_R, e->d_small0, b, K, P, c.vlad_final_l2_norm, p.vl_dR);
    if (rc) return rc;
    rc = xv_vlad_centers_backward(s, p.vl_n, p.vl_dR, cen, b, K, KG, P, c.weight_l2_regularizer, gptr(e, p.v_vlad_c));
    if (rc) return rc;
    rc = xv_vlad_pool_backward(s, a.a, p.vl_A, cen, p.vl_dR, b, Tp, P, K, KG, p.vl_dA, p.vl_dxv);
    if (rc) return rc;
    rc = xv_vlad_softmax_backward(s, p.vl_A, p.vl_dA, rows, KG, KGp, p.vl_dl);
    if (rc) return rc;
    rc = xv_colsum(s, p.vl_dl, rows, KG, KGp, gptr(e, p.v_vlad_b), e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xv_affine_wgrad_ld(s, a.a, rows, 1, P, 1, P, p.vl_dl, KGp, 1, 0, KGp, p.vl_wp, c.weight_l2_regularizer, p.vl_dwp, e->ws, e->ws_bytes);
    if (rc) return rc;
    rc = xv_vlad_repitch(s, p.vl_dwp, P, KG, KGp, gptr(e, p.v_vlad_w), KG);
    if (rc) return rc;
    rc = xv_affine_dgrad_ld(s, p.vl_dl, KGp, rows, 1, KGp, 1, p.vl_wp, e->bufD, P, e->ws, e->ws_bytes);
    if (rc) return rc;
    return xv_add_inplace(s, e->bufD, p.vl_dxv, (size_t)rows * P);
}

}  // namespace

int xvp_backward(xv_engine* e, hipStream_t s, const float** da) {
    *da = is_vlad(e) ? e->bufD : nullptr;
    if (is_att(e)) return backward_attention(e, s);
    return is_vlad(e) ? backward_vlad(e, s) : 0;
}

int xvp_backward_join(xv_engine* e, hipStream_t s) {      // the two paths into the key input
    return is_att(e) ? xv_add_inplace(s, e->bufD, e->pool_.bufA, (size_t)e->B * e->Tl[e->F] * e->L[e->F - 2].c_out) : 0;
}

int xvp_reg_loss(xv_engine* e, hipStream_t s) {
    if (!is_vlad(e)) return 0;
    for (int v : {e->pool_.v_vlad_w, e->pool_.v_vlad_c}) {      // pooling.py:245,256: the assignment kernel and every centre (ghosts included), not the bias
        int rc = xv_sumsq_ordered(s, vptr(e, v), e->vars[v].count, 0.5f * e->cfg.weight_l2_regularizer, e->scalars + 1, (float*)e->ws);
        if (rc) return rc;
    }
    return 0;
}

int xvp_endpoint(xv_engine* e, const std::string& n, const XvView& v) {
    XvPooling& p = e->pool_;
    const int Tp = e->Tl[e->F];
    // debug views of the backward scratch (valid right after backward stage 0)
    if (n == "debug:da5" && !is_vlad(e)) {     // evaluated on demand with the standalone pooling backward (valid after backward stage 0, before stage 1)
        XvAffine& a5 = e->L[e->F - 1];
        ActScope act(e, a5);
        int rc = xv_bn_apply(e->last_stream, a5.z, a5.rows, a5.c_out, a5.ldz, a5.scale, a5.shift, 1, a5.a, a5.c_out);
        if (rc) return rc;
        rc = xv_stat_pool_backward(e->last_stream, a5.a, p.pool, e->d_small0, e->B, Tp, p.P, e->bufD);
        if (rc) return rc;
        return v.set(e->bufD, e->B * Tp, p.P, p.P);
    }
    if (n == "debug:dpool") return v.set(e->d_small0, e->B, p.pool_dim, p.pool_dim);
    if (is_vlad(e)) {      // pooling.py:250,273-275
        if (n == "vlad_key") return v.set(p.vl_logits, e->B * Tp, p.VKG, p.VKGp);
        if (n == "vlad_weights") return v.set(p.vl_A, e->B * Tp, p.VKG, p.VKG);
        if (n == "vlad_centers") return v.set(vptr(e, p.v_vlad_c), p.VKG, p.P, p.P);
    }
    if (n == "attention_weights" && is_att(e)) return v.set(p.att_w, e->B, Tp, Tp);     // [b, heads = 1, frames]
    if (n == "att_key1_relu" && is_att(e) && e->L[e->K1()].act == 1) {      // relu key (type 1) lives inside the score kernels: rebuild on demand
        XvAffine& k1 = e->L[e->K1()];
        float* sc = xve_endpoint_scratch(e, (size_t)k1.rows * k1.c_out);
        if (!sc) return 1;
        int rc = xv_relu_backward(e->last_stream, k1.z, k1.z, (size_t)k1.rows * k1.c_out, sc);      // z > 0 ? z : 0
        if (rc) return rc;
        return v.set(sc, k1.rows, k1.c_out, k1.c_out);
    }
    if (n == "pooling") return v.set(p.pool, e->B, p.pool_dim, p.pool_dim);
    return XV_EP_UNKNOWN;
}
