// Engine state shared by the engine's translation units (private to csrc/): the variable table entry, the layer record, `struct xv_engine`,
// the amax slot layout, and the few helpers and functions more than one unit uses.  The units:
//   xv_engine.hip       create / destroy / bind / introspection, the variable table, the arena
//   xv_engine_fwd.hip   weight preparation, forward, loss forward, the regularisation loss
//   xv_engine_bwd.hip   streams, dz ring, join, stage events, layer backward in both precisions, the four backward stages
//   xv_engine_step.hip  the RCCL exchange, the update, loss pointers, endpoint views
//   xv_engine_pool.hip  the pooling layer (XvPooling): statistics, self-attention, ghost_vlad - one function per phase
//   xv_engine_head.hip  the loss head (XvHead): none, the softmax family, pairwise, GE2E - one function per phase
// The four units above read neither the pooling kind nor the head kind: they call the phase functions declared at the end of this header.
// No engine unit holds device code: every launch goes through a launcher of the kernel units (the unit headers below, include/xvector_hip.h).
//
// HBM layout (all fp32, channel axis contiguous):
//   variables  : caller-owned flat buffer, TF variable order, trainable first then BN moving
//                statistics; every variable starts on a 16-byte boundary.  Gradients mirror the
//                trainable section, so backward "stages" finish contiguous tail slices of the
//                gradient buffer and the host can all-reduce them while earlier layers still run.
//   activations: per frame layer z_l (pre-BN) and a_l (post BN+ReLU), [chunks*frames_l][C_l].
//   backward   : one da buffer and one dz buffer, ping-ponged down the stack; dz is stored with
//                k-1 zero frames around each chunk so the data gradient is the SAME spliced-view
//                GEMM as the forward pass (xv_gemm_nt.hip).
//   weights    : kernel-layout copies (transposed / tap-flipped / channel-padded) rebuilt once
//                per optimiser step.
#pragma once
#include <initializer_list>
#include <string>
#include <vector>

#include "xv_common.h"
#include "xv_bn.h"
#include "xv_ew.h"
#include "xv_gemm.h"
#include "xv_loss.h"
#include "xv_pool.h"
#include "xv_prep.h"
#include "xv_skinny.h"

struct XvVar {
    std::string name;
    int32_t shape[4];
    int32_t rank;
    size_t offset;   // floats, into the variables buffer
    size_t count;    // floats
    bool trainable;
};

struct XvAffine {   // one conv/dense layer (+ optional BN, ReLU)
    std::string prefix;    // "tdnn1"
    std::string kind;      // "conv" | "dense"
    int k, c_in, c_pad, c_out;
    bool has_bn, has_relu, fused_bn;
    int v_kernel, v_bias, v_gamma, v_beta, v_mmean, v_mvar;
    float *wt = nullptr, *wf = nullptr;   // kernel-layout weights (wf only when k > 1)
    float *z = nullptr, *a = nullptr;     // activations
    float *bn_part = nullptr, *mean = nullptr, *invstd = nullptr, *scale = nullptr, *shift = nullptr;
    // split precision (f16x3): fp16 planes of the kernel-layout weights and of this layer's BN+ReLU output
    unsigned short *wth = nullptr, *wfh = nullptr, *ah = nullptr;
    size_t wth_stride = 0, wfh_stride = 0;    // plane strides (elements)
    int o_ld = 0;                             // plane pitch of c_out (multiple of 8)
    int ldz = 0;                              // floats per row of z and of this layer's dz (= c_out except the pooled layer: rows on the 128-byte grid)
    float *zmin = nullptr, *zmax = nullptr;
    int rows;                             // rows of the most recent forward
    std::string scope;                    // variable scope under "tdnn/" ("" or "attention/att_key0/")
    int in_layer = -1;                    // index of the layer whose output this one reads (-1: the features / the pooled vector)
    int act = 0;                          // 3: tanh on the affine output (att_key_network_type 3), no BN
    int wslot = 0, aslot = 0;             // amax slots of the weights / of the BN+ReLU output planes
    int v_alpha = -1;                     // prelu: the layer's "<prefix>_relu/alpha" variable (network_relu_type, common.py:35-39)
};

constexpr int XV_Z_SLOTS = 16;

// What build_variables makes a layer record (and its variables) from
struct XvLayerSpec { std::string prefix; const char* kind; const char* scope; int k, cin, cout; bool bn, relu, fused; int in_layer, act; };

// The pooling layer between the last frame layer and tdnn(F+1): its kind, sizes, variables and every buffer only it uses (xv_engine_pool.hip)
struct XvPooling {
    int kind = XV_POOL_STATISTICS;        // xv_config.pooling
    int P = 0;                            // channels of the pooled (last frame) layer
    int pool_dim = 0;                     // columns of the pooled vector: 2 P, or K P with ghost_vlad
    int key_layers() const { return kind == XV_POOL_SELF_ATTENTION ? 2 : 0; }      // att_key0, att_key1 behind the segment layers in the layer table
    // ghost_vlad reads the last frame layer's activation twice: it is written like any other frame layer's (and its backward takes a materialised
    // d a); the other kinds apply BN + ReLU inside the pooling reduction
    bool writes_activation() const { return kind == XV_POOL_GHOST_VLAD; }
    // only the statistics-pooling kernels take the pooled layer's z with rows on the 128-byte grid (the other kinds' kernels take dense rows)
    bool z_on_row_grid() const { return kind == XV_POOL_STATISTICS; }
    int v_query = -1;
    // ghost_vlad pooling (xv_vlad.hip): K centres + G ghost clusters on the last frame layer's ReLU output.  The assignment GEMMs see W / the
    // logits / d logits with KGp = K + G rounded up to 4 columns (xv_vlad_repitch writes the copies of the variables with zero padding columns).
    int VK = 0, VG = 0, VKG = 0, VKGp = 0;
    int v_vlad_w = -1, v_vlad_b = -1, v_vlad_c = -1;
    float *vl_wp = nullptr, *vl_wt = nullptr, *vl_bp = nullptr, *vl_dwp = nullptr;       // [P][KGp], [KGp][P], [KGp], [P][KGp]
    float *vl_logits = nullptr, *vl_dl = nullptr;                                        // [B*T_pool][KGp]
    float *vl_A = nullptr, *vl_dA = nullptr;                                             // [B*T_pool][KG]
    float *vl_R = nullptr, *vl_dR = nullptr, *vl_n = nullptr;                            // [B][K][P] residuals, [B][K] assignment mass
    float* vl_dxv = nullptr;                                                             // [B*T_pool][P]: the value path of d x
    float *att_score = nullptr, *att_w = nullptr, *att_dw = nullptr, *att_ds = nullptr;   // [B*T5]
    float* bufA = nullptr;                // d (key input) through the key network, [B*T_pool][width of tdnn(F-1)]
    float* pool = nullptr;                // the pooled vector [B][pool_dim]
    float* pool_wpos = nullptr;           // [B][P] share of each chunk's frame weights on ReLU-active frames (pooling forward -> BN backward)
    float* pool_amax = nullptr;           // [B][P] each chunk's largest pooled activation
    bool pool_closed_form = true;         // the last frame layer's BN backward takes its reductions from the pooled statistics (plain ReLU)
};

// The loss head on the engine's output: its kind, sizes, variables, buffers and the state of the most recent loss (xv_engine_head.hip)
enum { XV_HEAD_NONE = 0, XV_HEAD_SOFTMAX, XV_HEAD_PAIR, XV_HEAD_GE2E };
struct XvHead {
    int kind = XV_HEAD_NONE;              // none: a predict-only engine | the softmax family (loss_kind 0..3) | pairwise (loss_kind 4 / 5, xv_triplet.hip) | GE2E (loss_kind 6, xv_triplet.hip)
    bool has_loss() const { return kind != XV_HEAD_NONE; }
    int N = 0, ldl = 0;                   // speakers (0: no softmax/output variables) and the logits pitch
    int v_loss_kernel = -1, v_loss_bias = -1, v_ring = -1;
    float *logits = nullptr, *dlogits = nullptr, *dnorm = nullptr, *row_loss = nullptr;
    float *inv_norm = nullptr, *wn = nullptr, *wnt = nullptr, *dwn = nullptr;
    float* xnorm = nullptr;               // [B] ||out[r]||, written with the loss rows
    float* mhe_coef = nullptr;            // [1 + 2*Lout]: g, u, v of the MHE auxiliary loss
    int32_t* mhe_counts = nullptr;        // [N] label histogram
    // pairwise heads: options from xv_engine_set_pair_loss
    bool pair_set = false, pair_e2e = false;      // pair_e2e: the last loss was the e2e validation loss (no backward)
    xv_pair_loss_config pair_cfg = {};
    float *pair_ws = nullptr, *pair_stats = nullptr;
    size_t pair_ws_bytes = 0;
    // the GE2E head: options from xv_engine_set_ge2e_loss, the trainable scalars ge2e/w and ge2e/b; it shares pair_ws / pair_stats / pair_e2e
    bool ge2e_set = false;
    xv_ge2e_config ge2e_cfg = {};
    int v_ge2e_w = -1, v_ge2e_b = -1;
    // the most recent loss
    int32_t* labels_dev = nullptr;        // caller's pointer of the current step
    float lambda = 0.f;
    int with_margin = 1;
};

struct xv_engine {
    xv_config cfg;
    std::vector<XvVar> vars;
    size_t n_train = 0, n_all = 0, n_opt = 0;
    float *V = nullptr, *G = nullptr, *S = nullptr;   // bound buffers
    // frame-level layers tdnn1..tdnnF (F = 5 in the reference, tdnn.py:35-127; any table of (context, width) in the extended
    // form), then the two segment-level layers tdnn(F+1), tdnn(F+2), then the attention key layers att_key0, att_key1
    std::vector<XvAffine> L;
    XvPooling pool_;
    XvHead head_;
    int F = 5;                            // frame-level layers
    int NL = 7;                           // layers in use
    int S0() const { return F; }          // index of the first segment-level layer (tdnn6 in the reference)
    int S1() const { return F + 1; }
    int K0() const { return F + 2; }      // attention key layers
    int K1() const { return F + 3; }
    int amax_a = 1, amax_wt = 0, amax_dz = 0;   // slot ranges inside `amax`, see amax layout below
    int min_frames = 15;                  // receptive field of the frame layers
    float* bwd_part = nullptr;            // BN-backward reduction partials written by a data-gradient GEMM epilogue
    int bwd_part_layer = -1, bwd_part_chunks = 0;   // ... for this layer's BN backward (-1: none pending)
    int c_pad0 = 0;
    int Lout = 0;
    // device arena
    char* arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    float *xpad = nullptr, *h7_buf = nullptr, *out_buf = nullptr;
    float *h7 = nullptr, *out = nullptr;   // views of the most recent forward (may alias tdnn7's z / h7)
    float *bufD = nullptr, *bufZ[XV_Z_SLOTS] = {}, *d_small0 = nullptr, *d_small1 = nullptr;
    // second stream: weight gradients run beside the data-gradient chain (they only share dz)
    hipStream_t side = nullptr;
    // third stream: the loss head's weight gradient (5 launches, ~0.1 ms alone) starts as soon as dlogits exist and never sits in
    // front of the segment layers' weight gradients on `side` (whose dz slots the main chain is waiting for)
    hipStream_t side2 = nullptr;
    void* ws_side2 = nullptr;
    bool stage_lw = false;        // deferred stage 0: its slice also needs ev_lw
    hipEvent_t ev_dz = nullptr, ev_lw = nullptr, ev_join = nullptr;
    hipEvent_t ev_prep = nullptr, ev_lossprep = nullptr;     // side-stream halves of ensure_weights
    bool prep_pending = false, lossprep_pending = false;
    hipEvent_t ev_comm = nullptr;                 // behind the most recent xv_engine_allreduce on the caller's communication stream
    bool comm_pending = false;
    hipEvent_t ev_stage[XV_BWD_STAGES][2] = {};   // [stage][0 main, 1 side]: that stage's gradients are complete (backward_async)
    bool stage_side[XV_BWD_STAGES] = {};          // the side-stream event of the stage was recorded
    // dz ping-pong state.  ring 0: the frame-level layers' dz (fp16 planes `dzh` in split precision) and, in fp32, every
    // layer's dz (`bufZ`); ring 1 (split precision only): the fp32 dz of the segment-level layers and the attention key
    // gradient in `bufZ` - its own ring, so a frame layer never waits for a segment layer's weight gradient.
    // [measured, same box] giving fp32 mode that second ring as well (it removes a 77 us wait of the last frame layer's BN backward
    // for the slot tdnn7's weight gradient reads) makes the step 0.07 ms SLOWER: the BN backward then runs beside the loss head's
    // side-stream chain and both crawl
    // fp32 mode has a slot per layer when the arena can afford it (`z_private`): no slot is rewritten inside a step, so the data-gradient
    // chain never waits for a weight gradient and the side stream records nothing per layer - every wait / record is a barrier packet
    // that costs the stream it sits on 5-6 us (profiles/r05_event_packets.txt).
    struct ZRing { int cur = 0, n = 2; bool pending[XV_Z_SLOTS] = {}; hipEvent_t ev[XV_Z_SLOTS] = {}; } zr[2];
    int nz = 2;                   // slots of bufZ
    bool z_private = false;       // nz covers every dz of a step
    bool side_dirty = false;      // weight-gradient work is on the side stream since the last join
    int z_taken = 0;              // slots handed to the side stream since the last join
    bool lw_pending = false;      // the loss head's weight gradient (side stream) - it reads no dz buffer, so it has its own event
    bool concurrent = true;
    void* ws_side = nullptr;
    float *scalars = nullptr;   // [0] raw loss, [1] reg loss, [2] grad sumsq
    // segment-level layers in one launch each (xv_skinny.hip) when the batch has <= XV_SEGMENT_MAX_ROWS chunks
    bool sk = true;                 // XV_SEGMENT_FUSED=0 keeps the GEMM / slab-sum / BatchNorm launches apart (A/B, and what B > 128 runs)
    uint32_t* sk_tickets = nullptr; // one per 32 output columns + the loss mean's
    size_t sk_ntickets = 0;
    float* lrelu_slope = nullptr;   // network_relu_type lrelu: a constant 0.2 vector as wide as the widest layer
    // split precision state
    bool f16 = false;
    unsigned short* xh = nullptr;             // planes of the (channel-padded) input features
    unsigned short* dzh[2] = {nullptr, nullptr};
    size_t dzh_halfs = 0;                     // halfs per plane of a dz buffer
    uint32_t* amax = nullptr;                 // [AMAX_SLOTS] float bits, see the amax layout below
    bool amax_wt_clean = false, amax_dz_clean = false;   // zeroed by the forward pass's one memset over the whole table
    void* ws = nullptr;
    size_t ws_bytes = 0;
    bool weights_dirty = true;
    const float* pad_src = nullptr;      // engine_forward -> prep_layers: the features whose channel padding rides on the first layer's weight-copy launch
    int pad_rows = 0;
    bool reg_valid = false;
    // state of the most recent forward
    int B = 0, T = 0, training = 0;
    int Tl[XV_MAX_FRAME_LAYERS + 1] = {};   // frames after each frame layer (index 0 = input)
    bool has_loss() const { return head_.has_loss(); }
    hipStream_t last_stream = nullptr;
    size_t stage_begin[XV_BWD_STAGES], stage_end[XV_BWD_STAGES];
    // scratch of the endpoints that are rebuilt on demand (xv_engine_endpoint: "<layer>_bn", "att_key1_relu"): a buffer of its own, allocated at
    // the first such request - every arena buffer wide enough holds live backward state (a dz slot per layer) between two passes
    float* ep_scratch = nullptr;
    size_t ep_scratch_floats = 0;
};

// amax layout (F = frame layers; groups on 16-byte boundaries): 0 input x | amax_a + [0, F): BN+ReLU outputs of tdnn1..F-1 and att_key0 (slot F-1) |
// amax_wt + [0, F+2): weights of tdnn1..F, att_key0/1 (both layouts share a slot) | amax_dz + [0, F+2): dz of the same layers
// (one slot per layer: zeroed once per backward pass, not once per layer)
enum { AMAX_X = 0, AMAX_SLOTS = 64 };
#define AMAX_A (e->amax_a)
#define AMAX_WT (e->amax_wt)
#define AMAX_DZ (e->amax_dz)

// frame-level layers (rows = chunks x frames): tdnn1..F and the attention key layers; the two layers after pooling are segment level
inline bool is_frame(const xv_engine* e, int i) { return i < e->F || i >= e->F + 2; }

inline float* vptr(xv_engine* e, int idx) { return e->V + e->vars[idx].offset; }
inline float* gptr(xv_engine* e, int idx) { return e->G + e->vars[idx].offset; }

// network_relu_type (tdnn.py:24-30): while in scope, the entry points that take a `relu` flag apply y > 0 ? y : slope[c] * y for this
// layer - prelu: slope = the layer's alpha variable (d alpha goes to its gradient slot), lrelu: the constant 0.2 vector (xv_ew.h)
struct ActScope {
    ActScope(xv_engine* e, const XvAffine& a) {
        if (!a.has_relu || e->cfg.relu_type == XV_RELU_RELU) return;
        if (e->cfg.relu_type == XV_RELU_PRELU) xv_set_act_context(vptr(e, a.v_alpha), e->G ? gptr(e, a.v_alpha) : nullptr);
        else xv_set_act_context(e->lrelu_slope, nullptr);
    }
    ~ActScope() { xv_set_act_context(nullptr, nullptr); }
};

// l2 weight of the loss head's kernel (output_weight_l2_regularizer, trainer.py:332-358: negative = the network's)
inline float xve_output_l2(const xv_config& c) { return c.output_weight_l2_regularizer >= 0.f ? c.output_weight_l2_regularizer : c.weight_l2_regularizer; }

// C[M][N] = A[M][K] . Bt[N][K]^T as a segment-level launch (xv_skinny.hip) on the engine's workspace and tickets; the caller adds
// the destination, the bias, the row term and the epilogue
inline XvSkinny xve_skinny(const xv_engine* e, const float* A, long lda, const float* Bt, long ldb, int M, int N, int K) {
    XvSkinny g = {};
    g.A = A; g.lda = lda; g.Bt = Bt; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.epi = XV_SK_PLAIN;
    g.ws = e->ws; g.ws_bytes = e->ws_bytes; g.tickets = e->sk_tickets;
    return g;
}

// What the arena layout depends on besides the layer table: row capacities, the backward ping-pong sizes, the GEMM workspace.
struct ArenaPlan {
    std::vector<size_t> rows;      // rows[i] = chunks x frames entering frame layer i; rows[F] = frames that are pooled
    size_t B = 0, maxc = 512, bufd = 0, bufz = 0, dzh_halfs = 0, ntick = 0, ws = 0;
    size_t lrows(const xv_engine* e, int i) const { return i < e->F ? rows[i + 1] : (i >= e->F + 2 ? rows[e->F] : B); }
};

// The cursor of a layout walk: 256-byte aligned buffers one behind the other.  Measuring (base == nullptr) only adds the sizes up;
// assigning also sets the pointers, and a buffer that would end behind the arena gets none (`ok` says so).
struct ArenaCursor {
    char* base = nullptr;
    size_t capacity = 0, used = 0;
    bool ok = true;
    template <class T> void operator()(T*& p, size_t floats) {
        const size_t bytes = xv_align(floats * sizeof(float), 256);
        if (base) {
            if (used + bytes > capacity) { p = nullptr; ok = false; return; }
            p = (T*)(base + used);
        }
        used += bytes;
    }
};

// A named view of the most recent forward, as xv_engine_endpoint hands it out.  The lookups of the pooling layer and of the loss head return
// 0 (served), XV_EP_UNKNOWN (not one of their names; no error text is set) or a launcher's error.
enum { XV_EP_UNKNOWN = 3 };
struct XvView {
    float** ptr; int32_t *rows, *cols, *ld;
    int set(float* p, int r, int c, int l) const { *ptr = p; *rows = r; *cols = c; *ld = l; return 0; }
};

// xv_engine.hip: appends a variable to the table (build_variables and the two declare phases); returns its index
int xve_add_var(xv_engine* e, const std::string& name, std::initializer_list<int> shape, bool trainable);
// xv_engine_fwd.hip: `s` waits for the side-stream halves of the weight preparation (no-ops when none is pending)
int xve_wait_prep(xv_engine* e, hipStream_t s);
int xve_wait_lossprep(xv_engine* e, hipStream_t s);
// xv_engine_fwd.hip: regularization_loss into scalars[1]
int xve_reg_loss(xv_engine* e, hipStream_t s);
// xv_engine_fwd.hip: forward of frame-level layer i (a frame layer or a key layer) over `segs` chunks of t_in frames
int xve_layer_forward(xv_engine* e, hipStream_t s, int i, int segs, int t_in);
// xv_engine_bwd.hip: `waiter` waits for everything enqueued so far on `signaller`; a slot of the fp32 dz ring (nullptr: the wait failed); the
// backward of one layer; the BatchNorm-backward epilogue of a segment-level launch
int xve_chain(hipStream_t signaller, hipStream_t waiter, hipEvent_t ev);
float* xve_take_dz(xv_engine* e, hipStream_t s);
#define XV_REQUIRE_SLOT(cond) XV_REQUIRE(cond, "engine_backward: waiting for a dz slot failed")
int xve_layer_backward(xv_engine* e, hipStream_t s, XvAffine& a, const float* da, const float* x, int segs, int t_in, float* dx, const float* act_out);
void xve_skinny_bn_backward(xv_engine* e, XvSkinny& g, XvAffine& a, float* dz);
// xv_engine_step.hip: scratch of the endpoints that are rebuilt on demand (nullptr: the error is set)
float* xve_endpoint_scratch(xv_engine* e, size_t floats);

// ---- the pooling layer, one function per phase (xv_engine_pool.hip)
int xvp_check_config(const xv_config* c);                                  // engine_create: the checks of the pooling fields
void xvp_configure(xv_engine* e);                                          // kind and sizes from e->cfg
void xvp_key_layers(const xv_engine* e, int c_key, std::vector<XvLayerSpec>& specs);   // appends the key layers it adds to the layer table
void xvp_declare_variables(xv_engine* e);                                  // at the pooling layer's place in graph order (behind the key layers)
void xvp_arena(xv_engine* e, const ArenaPlan& p, ArenaCursor& take);       // its buffers and the pooled vector
void xvp_arena_tail(xv_engine* e, const ArenaPlan& p, ArenaCursor& take);  // the per-chunk statistics at the arena's end
size_t xvp_workspace_bytes(const xv_engine* e, const ArenaPlan& p);
int xvp_forward(xv_engine* e, hipStream_t s, int b, int t, const int32_t* frames);      // the last frame layer's z / a -> pool
// d pool (d_small0) -> what the last frame layer's backward takes: *da = a materialised d a (bufD), or nullptr = the closed-form upstream
// xvp_upstream, which that layer's BatchNorm backward evaluates; xvp_backward_join, behind that layer, adds the key network's path into d (key input)
int xvp_backward(xv_engine* e, hipStream_t s, const float** da);
XvBnUpstream xvp_upstream(const xv_engine* e);
int xvp_backward_join(xv_engine* e, hipStream_t s);
int xvp_reg_loss(xv_engine* e, hipStream_t s);
int xvp_endpoint(xv_engine* e, const std::string& n, const XvView& v);

// ---- the loss head, one function per phase (xv_engine_head.hip, with xv_engine_set_pair_loss / xv_engine_set_ge2e_loss)
int xvh_check_config(const xv_config* c);                                  // engine_create: the checks of the loss fields
void xvh_configure(xv_engine* e);                                          // kind, N, ldl; the auxiliary losses this loss never reaches are cleared
void xvh_declare_variables(xv_engine* e);
void xvh_arena(xv_engine* e, const ArenaPlan& p, ArenaCursor& take);
void xvh_arena_tail(xv_engine* e, const ArenaPlan& p, ArenaCursor& take);
size_t xvh_workspace_bytes(const xv_engine* e, const ArenaPlan& p);
int xvh_prep_weights(xv_engine* e, hipStream_t s);                         // kernel-layout copies of the head's weights
int xvh_loss_forward(xv_engine* e, hipStream_t s, const int32_t* labels, int global_step);
int xvh_wgrad(xv_engine* e, hipStream_t s);                                // the head's weight gradient, on its own stream
// d out into d_small0.  *dz7_fused: the dz of tdnn7 when its BatchNorm backward rode on that launch (`sk`: the segment-level launches are in use)
int xvh_dout(xv_engine* e, hipStream_t s, bool sk, float** dz7_fused);
int xvh_ring_grad(xv_engine* e, hipStream_t s);
int xvh_reg_loss(xv_engine* e, hipStream_t s);
int xvh_endpoint(xv_engine* e, const std::string& n, const XvView& v);
