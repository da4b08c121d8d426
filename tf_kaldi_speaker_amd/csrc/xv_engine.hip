// Engine, life cycle: the whole tdnn (model/tdnn.py:33-191) + entire_network (model/trainer.py:168-188) + loss (model/loss.py) +
// regulariser/optimiser (model/trainer.py:332-436) graph as a fixed sequence of kernel launches; the native counterpart of what the TF1
// runtime does under sess.run(train_op) - the Python Trainer only feeds pointers.  This unit: what exists before the first step - argument
// checks of xv_engine_create, the variable table in TF order (build_variables), the device arena (one layout walk, measured then
// assigned), streams and events - and destroy / bind / introspection.  What a step launches is in xv_engine_fwd.hip, xv_engine_bwd.hip
// and xv_engine_step.hip; what the pooling layer and the loss head add to each phase in xv_engine_pool.hip and xv_engine_head.hip; the
// shared state in xv_engine.h.
#include <algorithm>

#include "xv_engine.h"

int xve_add_var(xv_engine* e, const std::string& name, std::initializer_list<int> shape, bool trainable) {
    XvVar v;
    v.name = name;
    v.rank = (int32_t)shape.size();
    v.count = 1;
    int i = 0;
    for (int s : shape) { v.shape[i++] = s; v.count *= (size_t)s; }
    for (; i < 4; ++i) v.shape[i] = 1;
    v.offset = 0;
    v.trainable = trainable;
    e->vars.push_back(v);
    return (int)e->vars.size() - 1;
}

namespace {

void build_variables(xv_engine* e) {
    const xv_config& c = e->cfg;
    const int D = c.feat_dim;
    e->Lout = c.num_nodes_last_layer;
    xvp_configure(e);
    xvh_configure(e);
    const int F = e->F, P = e->pool_.P;
    // slot groups start on 16-byte boundaries and are zeroed in multiples of 16 bytes: an unaligned / odd-sized hipMemsetAsync is split
    // into two fill kernels (~5 us each on the stream)
    e->amax_a = 4; e->amax_wt = 4 + (int)xv_align(F, 4); e->amax_dz = e->amax_wt + (int)xv_align(F + 2, 4);
    std::vector<XvLayerSpec> specs;
    {
        int cin = D;
        for (int i = 0; i < F; ++i) {
            const int k = c.num_frame_layers > 0 ? c.frame_context[i] : (i == 0 || i == 1 ? 5 : (i == 2 ? 7 : 1));
            const int w = c.num_frame_layers > 0 ? c.frame_width[i] : (i == F - 1 ? P : 512);
            // [TF] rank-4 inputs (the conv layers, tdnn.py:39-93) take the fused BN kernel: SURVEY N4
            specs.push_back({"tdnn" + std::to_string(i + 1), k > 1 ? "conv" : "dense", "", k, cin, w, true, true, k > 1, i - 1, 0});
            cin = w;
        }
    }
    const int Ckey = specs[F - 2].cout;      // the attention key network reads the last-but-one frame layer (tdnn4_relu in the shipped configs)
    specs.push_back({"tdnn" + std::to_string(F + 1), "dense", "", 1, e->pool_.pool_dim, 512, true, true, false, -1, 0});
    specs.push_back({"tdnn" + std::to_string(F + 2), "dense", "", 1, 512, e->Lout, !c.last_layer_no_bn, !c.last_layer_linear, false, F, 0});
    xvp_key_layers(e, Ckey, specs);
    e->NL = (int)specs.size();
    e->L.assign(e->NL, XvAffine());
    // graph-construction order of the reference: the frame layers, the pooling layer's key layers and variables, the segment layers
    std::vector<int> order;
    for (int i = 0; i < F; ++i) order.push_back(i);
    for (int i = F + 2; i < e->NL; ++i) order.push_back(i);
    order.push_back(F); order.push_back(F + 1);
    for (int i : order) {
        if (i == F) xvp_declare_variables(e);
        XvAffine& a = e->L[i];
        const XvLayerSpec& s = specs[i];
        a.prefix = s.prefix; a.kind = s.kind; a.scope = s.scope; a.in_layer = s.in_layer; a.act = s.act;
        a.k = s.k; a.c_in = s.cin; a.c_out = s.cout;
        // operand pitch: 16-byte chunks of fp16 planes need multiples of 8 (feature layer 30 -> 32, att_key1 1500 -> 1504)
        a.c_pad = (int)xv_align(s.cin, (i == 0 || (e->f16 && is_frame(e, i))) ? 8 : 4);
        a.o_ld = (int)xv_align(s.cout, 8);
        // The pooled layer's pre-BN tensor and its gradient are the largest tensors of the step and are streamed by HBM-bound kernels (pooling, the
        // pooled BatchNorm backward) and by the GEMMs' LDS-DMA: 1 500 channels = 6 000-byte rows start off the 128-byte grid (nine cache lines
        // per KiB instead of eight).  Plain fp32 path with statistics pooling and a plain ReLU only (the kernels of the other paths take dense rows).
        a.ldz = (i == F - 1 && !e->f16 && e->pool_.z_on_row_grid() && c.relu_type == XV_RELU_RELU && s.k == 1) ? (int)xv_align(s.cout, 32) : s.cout;
        a.has_bn = s.bn; a.has_relu = s.relu; a.fused_bn = s.fused;
        a.wslot = i < F ? i : i - 2;          // amax slots of the weights: tdnn1..F -> 0..F-1, att_key0/1 -> F, F+1
        a.aslot = i < F ? i : F - 1;          // BN+ReLU output planes: tdnn1..F-1 -> 0..F-2, att_key0 -> F-1
        std::string base = std::string("tdnn/") + s.scope + s.prefix + "_" + s.kind;
        if (s.k > 1) a.v_kernel = xve_add_var(e, base + "/kernel", {1, s.k, s.cin, s.cout}, true);
        else a.v_kernel = xve_add_var(e, base + "/kernel", {s.cin, s.cout}, true);
        a.v_bias = xve_add_var(e, base + "/bias", {s.cout}, true);
        a.v_gamma = a.v_beta = a.v_mmean = a.v_mvar = -1;
        if (s.bn) {
            std::string bn = std::string("tdnn/") + s.scope + s.prefix + "_bn";
            a.v_gamma = xve_add_var(e, bn + "/gamma", {s.cout}, true);
            a.v_beta = xve_add_var(e, bn + "/beta", {s.cout}, true);
            a.v_mmean = xve_add_var(e, bn + "/moving_mean", {s.cout}, false);
            a.v_mvar = xve_add_var(e, bn + "/moving_variance", {s.cout}, false);
        }
        if (c.relu_type == XV_RELU_PRELU && s.relu)      // prelu(x, name): variable_scope("<prefix>_relu") / "alpha" [C], common.py:35-39
            a.v_alpha = xve_add_var(e, std::string("tdnn/") + s.scope + s.prefix + "_relu/alpha", {s.cout}, true);
    }
    e->c_pad0 = e->L[0].c_pad;
    xvh_declare_variables(e);
    // offsets: trainable section first (graph order), then non-trainable; 16-byte aligned starts
    size_t off = 0;
    for (auto& v : e->vars) if (v.trainable) { v.offset = off; off += xv_align(v.count, 4); }
    e->n_train = off;
    for (auto& v : e->vars) if (!v.trainable) { v.offset = off; off += xv_align(v.count, 4); }
    e->n_all = off;
    e->n_opt = c.optimizer == 0 ? 0 : (c.optimizer == 1 ? e->n_train : 2 * e->n_train);

    // backward stages -> contiguous gradient ranges (stage 0 finishes the tail of the buffer)
    auto first_off = [&](int layer) { return e->vars[e->L[layer].v_kernel].offset; };
    // stage 0: segment layers + loss | 1: the last two frame layers (+ attention keys, created between them and the segment
    // layers) | 2: the middle frame layers | 3: the first two (reference F = 5: tdnn4-5 | tdnn3 | tdnn1-2)
    const int lo = F >= 4 ? 2 : 1;                                     // first layer of stage 2
    e->stage_begin[0] = first_off(F);     e->stage_end[0] = e->n_train;
    e->stage_begin[1] = first_off(F - 2); e->stage_end[1] = first_off(F);
    e->stage_begin[2] = first_off(lo);    e->stage_end[2] = first_off(F - 2);
    e->stage_begin[3] = 0;                e->stage_end[3] = first_off(lo);
}

// THE arena layout: every buffer, its size (in floats - the half-typed ones too: two planes of halfs are one float per element) and
// the condition under which it exists, in address order.  alloc_buffers runs it twice, to measure and to assign.
void arena_layout(xv_engine* e, const ArenaPlan& p, ArenaCursor& take) {
    const int F = e->F;
    const size_t B = p.B;
    take(e->xpad, p.rows[0] * e->c_pad0);
    for (int i = 0; i < e->NL; ++i) {
        XvAffine& a = e->L[i];
        const size_t r = p.lrows(e, i);
        take(a.wt, (size_t)a.c_out * a.k * a.c_pad);
        if (a.k > 1) take(a.wf, (size_t)a.c_in * a.k * a.c_out);
        take(a.z, r * a.ldz);
        take(a.a, r * a.c_out);
        take(a.bn_part, 4 * (size_t)xv_cdiv(r, XV_TILE_M) * a.c_out);
        take(a.mean, a.c_out); take(a.invstd, a.c_out);
        take(a.scale, a.c_out); take(a.shift, a.c_out);
        a.rows = 0;
    }
    if (e->f16) {
        take(e->xh, p.rows[0] * e->c_pad0);
        for (int i = 0; i < e->NL; ++i) {
            if (!is_frame(e, i)) continue;
            XvAffine& a = e->L[i];
            a.wth_stride = (size_t)a.c_out * a.k * a.c_pad;
            take(a.wth, a.wth_stride);
            if (i > 0) {
                a.wfh_stride = (size_t)a.c_in * a.k * a.o_ld;
                take(a.wfh, a.wfh_stride);
            }
            if (i < F - 1 || i == F + 2) take(a.ah, p.lrows(e, i) * a.o_ld);
            take(a.zmin, a.c_out);
            take(a.zmax, a.c_out);
        }
        take(e->amax, AMAX_SLOTS);
    }
    xvp_arena(e, p, take);      // the pooling layer's buffers, the pooled vector
    take(e->h7_buf, B * e->Lout);
    take(e->out_buf, B * e->Lout);
    xvh_arena(e, p, take);      // the loss head's buffers
    take(e->bufD, p.bufd);
    for (int i = 0; i < e->nz; ++i) take(e->bufZ[i], p.bufz);
    if (e->f16) {
        take(e->bwd_part, (size_t)xv_cdiv(p.rows[1], XV_TILE_M) * 3 * p.maxc);
        take(e->dzh[0], p.dzh_halfs);
        take(e->dzh[1], p.dzh_halfs);
    }
    const size_t small = B * (size_t)(e->pool_.pool_dim > 512 ? e->pool_.pool_dim : 512);
    take(e->d_small0, small);
    take(e->d_small1, small);
    take(e->scalars, 16);
    take(e->lrelu_slope, xv_align(p.maxc, 4) + 4);
    take(e->sk_tickets, p.ntick);       // zero (arena memset); every launch leaves them zero
    xvh_arena_tail(e, p, take);
    xvp_arena_tail(e, p, take);
    take(e->ws, p.ws / sizeof(float));
    take(e->ws_side, p.ws / sizeof(float));
    take(e->ws_side2, p.ws / sizeof(float));
}

// GEMM split slabs: weight-gradient partials dominate
size_t workspace_bytes(const xv_engine* e, const ArenaPlan& p) {
    size_t ws = 0;
    for (int i = 0; i < e->NL; ++i) {
        const XvAffine& a = e->L[i];
        size_t r = p.lrows(e, i);
        int M = a.k * a.c_pad, Nn = a.c_out;
        size_t s = (size_t)xv_tn_splits(M, Nn, (int)r) * M * Nn * sizeof(float);
        if (s > ws) ws = s;
        if (e->f16 && is_frame(e, i)) {
            s = (size_t)xv_tn16_splits(M, a.o_ld, (int)r) * M * a.o_ld * sizeof(float);
            if (s > ws) ws = s;
        }
    }
    ws = std::max(ws, std::max(xvh_workspace_bytes(e, p), xvp_workspace_bytes(e, p)));
    return xv_align(ws, 256);
}

int alloc_buffers(xv_engine* e) {
    const xv_config& c = e->cfg;
    const size_t B = c.max_batch, T = c.max_frames;
    const int F = e->F;
    int field = 1;
    for (int i = 0; i < F; ++i) field += e->L[i].k - 1;
    e->min_frames = field;
    XV_REQUIRE(B >= 1 && (int)T >= field, "engine: max_batch >= 1 and max_frames >= %d required (receptive field of the frame layers)", field);
    ArenaPlan p;
    p.B = B;
    p.rows.resize(F + 1);
    {
        size_t t_cur = T;
        p.rows[0] = B * T;
        for (int i = 0; i < F; ++i) { t_cur -= (size_t)(e->L[i].k - 1); p.rows[i + 1] = B * t_cur; }
        if (c.max_rows > 0) {     // row capacity given: any (chunks, frames) with chunks * frames <= max_rows (one chunk loses the fewest frames)
            XV_REQUIRE(c.max_rows >= field, "engine: max_rows %d is below the receptive field %d", c.max_rows, field);
            for (int i = 0; i <= F; ++i) p.rows[i] = std::min<size_t>(p.rows[i], (size_t)c.max_rows);
        }
    }
    // widest frame-level tensor (channels) and the ping-pong buffers of the backward pass: bufD holds d(layer output) /
    // d(layer input) ([rows][c]), bufZ a dz with k-1 zero frames around every chunk
    size_t max_pad_rows = 0;
    for (int i = 0; i < e->NL; ++i) {
        if (!is_frame(e, i)) continue;
        const XvAffine& a = e->L[i];
        p.maxc = std::max<size_t>(p.maxc, (size_t)a.c_out);
        p.maxc = std::max<size_t>(p.maxc, (size_t)a.c_in);
        const size_t r_out = p.lrows(e, i), r_in = i < F ? p.rows[i] : p.rows[F];
        p.bufd = std::max(p.bufd, std::max(r_out * a.c_out, r_in * (size_t)a.c_in));
        const size_t padded = r_out + B * 2 * (size_t)(a.k - 1);
        p.bufz = std::max(p.bufz, padded * (size_t)a.ldz);
        max_pad_rows = std::max(max_pad_rows, padded);
    }
    // a dz slot per layer (+ the attention key gradient) while that stays below 6 GiB (S5, the extended model at 128 x 400: 4.3 GB); the two-slot
    // ring otherwise - an engine sized for batched extraction (hundreds of thousands of rows, never a backward pass) does not pay for the slots
    e->nz = 2;
    {
        const XvEnv* env = xv_env();
        if (!env) return 2;
        // ... and only an engine with a loss head can run one: a predict-only engine (num_speakers == 0; Trainer.predict_batch builds them with
        // 49 152 rows) keeps the two slots - nine would be 2 GB of arena nothing ever reads
        if (env->dz_slots != 2 && !e->f16 && e->has_loss() && e->NL + 2 <= XV_Z_SLOTS && (size_t)(e->NL + 2) * p.bufz * sizeof(float) <= ((size_t)6 << 30))
            e->nz = e->NL + 2;
    }
    e->z_private = e->nz > 2;
    e->zr[0].n = e->f16 ? 2 : e->nz;
    e->zr[1].n = 2;
    p.dzh_halfs = xv_align(max_pad_rows * (size_t)xv_align(p.maxc, 8), 8);
    p.ntick = xv_skinny_tickets((int)std::max<size_t>(std::max<size_t>(e->head_.N, (size_t)e->pool_.pool_dim), std::max<size_t>(p.maxc, (size_t)e->Lout))) + 8;
    p.ws = workspace_bytes(e, p);
    ArenaCursor measured;
    arena_layout(e, p, measured);
    const size_t need = measured.used + 8192;
    XV_CHECK_HIP(hipMalloc((void**)&e->arena, need));
    XV_CHECK_HIP(hipMemset(e->arena, 0, need));
    e->arena_bytes = need;
    ArenaCursor assigned;
    assigned.base = e->arena; assigned.capacity = need;
    arena_layout(e, p, assigned);
    e->arena_used = assigned.used;
    XV_REQUIRE(assigned.ok && e->arena_used == measured.used, "engine: internal arena accounting error");
    if (e->f16) e->dzh_halfs = p.dzh_halfs;
    e->sk_ntickets = p.ntick;
    e->ws_bytes = p.ws;
    if (c.relu_type == XV_RELU_LRELU) {
        std::vector<float> h(xv_align(p.maxc, 4) + 4, 0.2f);      // tf.nn.leaky_relu default alpha
        XV_CHECK_HIP(hipMemcpy(e->lrelu_slope, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    {
        const XvEnv* env = xv_env();
        if (!env) return 2;
        e->sk = env->segment_fused != 0;
    }
    {   // lowest priority: the weight-gradient GEMMs are filler work; the small kernels of the critical
        // data-gradient chain must not queue behind their workgroups
        int least = 0, greatest = 0;
        XV_CHECK_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        XV_CHECK_HIP(hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, least));
        XV_CHECK_HIP(hipStreamCreateWithPriority(&e->side2, hipStreamNonBlocking, least));
    }
    // Events between the engine's own streams order kernels of ONE device: no system-scope fence (cache write-back towards the host and
    // peers) when they are recorded.  Which events carry the system-scope release: ev_join (end of a pass / of a non-deferred stage), ev_stage[][],
    // ev_lw and ev_comm - everything a collective, whose bytes peer GPUs read, may be ordered behind.  Device scope only: ev_dz, the ring
    // events, ev_prep, ev_lossprep (hand-overs between this engine's own kernels).
    const unsigned local = hipEventDisableTiming | hipEventDisableSystemFence;
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_dz, local));
    for (int r = 0; r < 2; ++r)
        for (int i = 0; i < e->zr[r].n; ++i) XV_CHECK_HIP(hipEventCreateWithFlags(&e->zr[r].ev[i], local));
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_lw, hipEventDisableTiming));      // (xv_engine_stage_wait: a collective's stream may wait on it)
    // ev_join is what makes the side streams' weight gradients visible to `s` at the end of a (non-deferred) stage, and a collective enqueued on
    // `s` next hands those bytes to PEER GPUs: it keeps the system-scope release (one packet per pass), like the stage / communication events
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_comm, hipEventDisableTiming));
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_prep, local));
    XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_lossprep, local));
    for (int k = 0; k < XV_BWD_STAGES; ++k)
        for (int j = 0; j < 2; ++j) XV_CHECK_HIP(hipEventCreateWithFlags(&e->ev_stage[k][j], hipEventDisableTiming));
    return 0;
}

}  // namespace

extern "C" int xv_engine_create(const xv_config* cfg, xv_engine** out) {
    XV_REQUIRE(cfg && out, "engine_create: null argument");
    if (!xv_env()) return 2;      // an environment switch this library does not know, or a value it does not understand: refused by name
    // the struct of ABI version 3 before the ghost_vlad fields were added behind it is still accepted (those fields then read as 0)
    const int32_t v3_bytes = (int32_t)offsetof(xv_config, vlad_num_centers);
    XV_REQUIRE(cfg->struct_bytes == (int32_t)sizeof(xv_config) || cfg->struct_bytes == v3_bytes,
               "engine_create: xv_config.struct_bytes is %d, this library's xv_config has %d bytes (ABI version %d): rebuild the host against include/xvector_hip.h",
               cfg->struct_bytes, (int)sizeof(xv_config), XV_ABI_VERSION);
    xv_config full;
    memset(&full, 0, sizeof(full));
    memcpy(&full, cfg, (size_t)cfg->struct_bytes);
    full.struct_bytes = (int32_t)sizeof(xv_config);
    cfg = &full;
    XV_REQUIRE(cfg->feat_dim > 0, "engine_create: feat_dim must be positive");
    XV_REQUIRE(cfg->num_nodes_pooling_layer > 0 && cfg->num_nodes_pooling_layer % 4 == 0,
               "engine_create: num_nodes_pooling_layer must be a positive multiple of 4 (got %d)", cfg->num_nodes_pooling_layer);
    XV_REQUIRE(cfg->num_nodes_last_layer > 0 && cfg->num_nodes_last_layer % 4 == 0,
               "engine_create: num_nodes_last_layer must be a positive multiple of 4 (got %d)", cfg->num_nodes_last_layer);
    if (int rc = xvh_check_config(cfg)) return rc;
    XV_REQUIRE(cfg->optimizer >= 0 && cfg->optimizer <= 2, "Optimizer %d is not supported.", cfg->optimizer);
    XV_REQUIRE(!cfg->feature_norm || cfg->feature_scaling_factor > 0.f, "If feature normalization is applied, scaling factor is necessary.");
    XV_REQUIRE(cfg->precision == XV_PRECISION_F32 || cfg->precision == XV_PRECISION_F16X3, "engine_create: unknown precision %d", cfg->precision);
    if (int rc = xvp_check_config(cfg)) return rc;
    if (cfg->num_frame_layers != 0) {       // extended frame-layer table (no reference counterpart: tdnn.py hard-codes 5 layers)
        XV_REQUIRE(cfg->num_frame_layers >= 3 && cfg->num_frame_layers <= XV_MAX_FRAME_LAYERS,
                   "engine_create: num_frame_layers must be 0 (the reference's 5) or 3..%d (got %d)", XV_MAX_FRAME_LAYERS, cfg->num_frame_layers);
        for (int i = 0; i < cfg->num_frame_layers; ++i) {
            XV_REQUIRE(cfg->frame_context[i] >= 1 && cfg->frame_context[i] <= 15, "engine_create: frame_context[%d] = %d is outside 1..15", i, cfg->frame_context[i]);
            XV_REQUIRE(cfg->frame_width[i] > 0 && cfg->frame_width[i] % 4 == 0, "engine_create: frame_width[%d] = %d must be a positive multiple of 4", i,
                       cfg->frame_width[i]);
        }
        XV_REQUIRE(cfg->frame_width[cfg->num_frame_layers - 1] == cfg->num_nodes_pooling_layer,
                   "engine_create: the last frame layer is the pooling layer: frame_width[%d] must equal num_nodes_pooling_layer", cfg->num_frame_layers - 1);
    }
    XV_REQUIRE(cfg->relu_type >= XV_RELU_RELU && cfg->relu_type <= XV_RELU_LRELU, "engine_create: unknown network_relu_type code %d", cfg->relu_type);
    xv_engine* e = new xv_engine();
    e->cfg = *cfg;
    e->F = cfg->num_frame_layers > 0 ? cfg->num_frame_layers : 5;
    e->f16 = cfg->precision == XV_PRECISION_F16X3;
    build_variables(e);
    int rc = alloc_buffers(e);
    if (rc) { xv_engine_destroy(e); return rc; }
    *out = e;
    return 0;
}

extern "C" void xv_engine_destroy(xv_engine* e) {
    if (!e) return;
    if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
    if (e->side2) { (void)hipStreamSynchronize(e->side2); (void)hipStreamDestroy(e->side2); }
    if (e->ev_dz) (void)hipEventDestroy(e->ev_dz);
    for (int r = 0; r < 2; ++r)
        for (int i = 0; i < XV_Z_SLOTS; ++i) if (e->zr[r].ev[i]) (void)hipEventDestroy(e->zr[r].ev[i]);
    if (e->ev_lw) (void)hipEventDestroy(e->ev_lw);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->ev_comm) (void)hipEventDestroy(e->ev_comm);
    if (e->ev_prep) (void)hipEventDestroy(e->ev_prep);
    if (e->ev_lossprep) (void)hipEventDestroy(e->ev_lossprep);
    for (int k = 0; k < XV_BWD_STAGES; ++k)
        for (int j = 0; j < 2; ++j) if (e->ev_stage[k][j]) (void)hipEventDestroy(e->ev_stage[k][j]);

    if (e->arena) (void)hipFree(e->arena);
    if (e->ep_scratch) (void)hipFree(e->ep_scratch);
    delete e;
}

extern "C" int xv_engine_num_variables(const xv_engine* e) { return e ? (int)e->vars.size() : 0; }

extern "C" int xv_engine_variable_info(const xv_engine* e, int index, const char** name, int32_t shape[4], int32_t* rank, size_t* offset,
                                       int32_t* trainable) {
    XV_REQUIRE(e && index >= 0 && index < (int)e->vars.size(), "variable_info: index out of range");
    const XvVar& v = e->vars[index];
    if (name) *name = v.name.c_str();
    if (shape) for (int i = 0; i < 4; ++i) shape[i] = v.shape[i];
    if (rank) *rank = v.rank;
    if (offset) *offset = v.offset;
    if (trainable) *trainable = v.trainable ? 1 : 0;
    return 0;
}

extern "C" size_t xv_engine_arena_bytes(const xv_engine* e) { return e ? e->arena_bytes : 0; }
extern "C" size_t xv_engine_variables_count(const xv_engine* e) { return e ? e->n_all : 0; }
extern "C" size_t xv_engine_trainable_count(const xv_engine* e) { return e ? e->n_train : 0; }
extern "C" size_t xv_engine_optimizer_state_count(const xv_engine* e) { return e ? e->n_opt : 0; }

extern "C" int xv_engine_bind(xv_engine* e, float* variables, float* grads, float* opt_state) {
    XV_REQUIRE(e && variables, "engine_bind: variables buffer required");
    XV_REQUIRE(((uintptr_t)variables % 16) == 0 && ((uintptr_t)grads % 16) == 0, "engine_bind: buffers must be 16-byte aligned");
    e->V = variables; e->G = grads; e->S = opt_state;
    e->weights_dirty = true;
    return 0;
}

extern "C" int xv_engine_set_concurrency(xv_engine* e, int enabled) {
    XV_REQUIRE(e, "null engine");
    e->concurrent = enabled != 0;
    return 0;
}

extern "C" int xv_engine_invalidate_weights(xv_engine* e) {
    XV_REQUIRE(e, "null engine");
    e->weights_dirty = true;
    return 0;
}
