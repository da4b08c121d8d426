// Engine state shared by the engine's translation units (private to csrc/): the variable table entry, the layer record, `struct xv_engine`,
// the amax slot layout, and the few helpers and functions more than one unit uses.  The units:
//   xv_engine.hip       create / destroy / bind / introspection, the variable table, the arena
//   xv_engine_fwd.hip   weight preparation, forward, loss forward, the regularisation loss
//   xv_engine_bwd.hip   streams, dz ring, join, stage events, layer backward in both precisions, the four backward stages
//   xv_engine_step.hip  the RCCL exchange, the update, loss pointers, endpoint views
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

struct xv_engine {
    xv_config cfg;
    std::vector<XvVar> vars;
    size_t n_train = 0, n_all = 0, n_opt = 0;
    float *V = nullptr, *G = nullptr, *S = nullptr;   // bound buffers
    // frame-level layers tdnn1..tdnnF (F = 5 in the reference, tdnn.py:35-127; any table of (context, width) in the extended
    // form), then the two segment-level layers tdnn(F+1), tdnn(F+2), then the attention key layers att_key0, att_key1
    std::vector<XvAffine> L;
    int F = 5;                            // frame-level layers
    int NL = 7;                           // layers in use
    int S0() const { return F; }          // index of the first segment-level layer (tdnn6 in the reference)
    int S1() const { return F + 1; }
    int K0() const { return F + 2; }      // attention key layers
    int K1() const { return F + 3; }
    int amax_a = 1, amax_wt = 0, amax_dz = 0;   // slot ranges inside `amax`, see amax layout below
    bool att = false;
    int v_query = -1;
    // ghost_vlad pooling (xv_vlad.hip): K centres + G ghost clusters on the last frame layer's ReLU output, which is then written like any
    // other frame layer's (a) and whose backward takes a materialised d a.  The assignment GEMMs see W / the logits / d logits with
    // KGp = K + G rounded up to 4 columns (xv_vlad_repitch writes the copies of the variables with zero padding columns).
    bool vlad = false;
    int VK = 0, VG = 0, VKG = 0, VKGp = 0;
    int v_vlad_w = -1, v_vlad_b = -1, v_vlad_c = -1;
    float *vl_wp = nullptr, *vl_wt = nullptr, *vl_bp = nullptr, *vl_dwp = nullptr;       // [P][KGp], [KGp][P], [KGp], [P][KGp]
    float *vl_logits = nullptr, *vl_dl = nullptr;                                        // [B*T_pool][KGp]
    float *vl_A = nullptr, *vl_dA = nullptr;                                             // [B*T_pool][KG]
    float *vl_R = nullptr, *vl_dR = nullptr, *vl_n = nullptr;                            // [B][K][P] residuals, [B][K] assignment mass
    float* vl_dxv = nullptr;                                                             // [B*T_pool][P]: the value path of d x
    int pool_dim = 0;                     // columns of the pooled vector: 2 P, or K P with ghost_vlad
    float *att_score = nullptr, *att_w = nullptr, *att_dw = nullptr, *att_ds = nullptr;   // [B*T5]
    float* bufA = nullptr;                // d (key input) through the key network, [B*T_pool][width of tdnn(F-1)]
    int min_frames = 15;                  // receptive field of the frame layers
    float* bwd_part = nullptr;            // BN-backward reduction partials written by a data-gradient GEMM epilogue
    int bwd_part_layer = -1, bwd_part_chunks = 0;   // ... for this layer's BN backward (-1: none pending)
    int v_loss_kernel = -1, v_loss_bias = -1, v_ring = -1;
    float* mhe_coef = nullptr;            // [1 + 2*Lout]: g, u, v of the MHE auxiliary loss
    int32_t* mhe_counts = nullptr;        // [N] label histogram
    int c_pad0 = 0;
    int P = 0, Lout = 0, N = 0, ldl = 0;
    // device arena
    char* arena = nullptr;
    size_t arena_bytes = 0, arena_used = 0;
    float *xpad = nullptr, *pool = nullptr, *h7_buf = nullptr, *out_buf = nullptr;
    float *h7 = nullptr, *out = nullptr;   // views of the most recent forward (may alias tdnn7's z / h7)
    float *logits = nullptr, *dlogits = nullptr, *dnorm = nullptr, *row_loss = nullptr;
    float *inv_norm = nullptr, *wn = nullptr, *wnt = nullptr, *dwn = nullptr;
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
    float* xnorm = nullptr;         // [B] ||out[r]||, written with the loss rows
    float* pool_wpos = nullptr;     // [B][P] share of each chunk's frame weights on ReLU-active frames (pooling forward -> BN backward)
    float* pool_amax = nullptr;     // [B][P] each chunk's largest pooled activation
    bool pool_closed_form = true;   // the last frame layer's BN backward takes its reductions from the pooled statistics (plain ReLU)
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
    int32_t* labels_dev = nullptr;   // caller's pointer of the current step
    bool weights_dirty = true;
    const float* pad_src = nullptr;      // engine_forward -> prep_layers: the features whose channel padding rides on the first layer's weight-copy launch
    int pad_rows = 0;
    bool reg_valid = false;
    // state of the most recent forward
    int B = 0, T = 0, training = 0;
    int Tl[XV_MAX_FRAME_LAYERS + 1] = {};   // frames after each frame layer (index 0 = input)
    float lambda = 0.f;
    int with_margin = 1;
    // pairwise loss heads (loss_kind 4 / 5, xv_triplet.hip): N = 0 (no softmax/output variables), options from xv_engine_set_pair_loss
    bool pair = false, pair_set = false, pair_e2e = false;      // pair_e2e: the last loss was the e2e validation loss (no backward)
    xv_pair_loss_config pair_cfg = {};
    float *pair_ws = nullptr, *pair_stats = nullptr;
    size_t pair_ws_bytes = 0;
    bool has_loss() const { return N > 0 || pair; }
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

// xv_engine_fwd.hip: `s` waits for the side-stream halves of the weight preparation (no-ops when none is pending)
int xve_wait_prep(xv_engine* e, hipStream_t s);
int xve_wait_lossprep(xv_engine* e, hipStream_t s);
// xv_engine_fwd.hip: regularization_loss into scalars[1]
int xve_reg_loss(xv_engine* e, hipStream_t s);
