// Engine, the rest of a step: the gradient exchange for hosts without torch.distributed (RCCL resolved at run time), the update
// (clip-by-global-norm + optimiser; the kernels are in xv_update.hip), the loss scalars, and the named views of the most recent
// forward (xv_engine_endpoint), some of which are rebuilt on demand.
#include <dlfcn.h>

#include <string>

#include "xv_engine.h"

// ---- gradient exchange for hosts without torch.distributed (the Python host runs the same collective through
// torch.distributed in parallel.py).  RCCL is resolved at first use from the process - the host that created the communicator has it
// loaded, and the communicator must be used with the library that made it - and only then from the default library path: this library
// has no link-time dependency on RCCL and loads on a box without it.
namespace {
typedef int (*rccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*rccl_errstr_fn)(int);
struct Rccl { rccl_allreduce_fn allreduce = nullptr; rccl_errstr_fn errstr = nullptr; bool tried = false; };
Rccl& rccl() {
    static Rccl r;
    if (!r.tried) {
        r.tried = true;
        void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
        void* h = nullptr;
        if (!sym) {
            for (const char* name : {"librccl.so.1", "librccl.so"}) {
                h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (h) break;
            }
            if (h) sym = dlsym(h, "ncclAllReduce");
        }
        r.allreduce = (rccl_allreduce_fn)sym;
        r.errstr = (rccl_errstr_fn)(h ? dlsym(h, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
    }
    return r;
}
}  // namespace

extern "C" int xv_engine_allreduce(xv_engine* e, void* comm_stream, int stage, void* rccl_comm) {
    XV_REQUIRE(e && e->G && rccl_comm && stage >= 0 && stage < XV_BWD_STAGES, "engine_allreduce: bad arguments (stage %d)", stage);
    Rccl& r = rccl();
    XV_REQUIRE(r.allreduce, "engine_allreduce: ncclAllReduce is not available in this process (load RCCL - it made the communicator - first)");
    int rc = xv_engine_stage_wait(e, comm_stream, stage);
    if (rc) return rc;
    const size_t begin = e->stage_begin[stage], count = e->stage_end[stage] - begin;
    if (count > 0) {
        const int nr = r.allreduce(e->G + begin, e->G + begin, count, 7 /* ncclFloat32 */, 0 /* ncclSum */, rccl_comm, (hipStream_t)comm_stream);
        XV_REQUIRE(nr == 0, "engine_allreduce: ncclAllReduce of stage %d (%zu floats) failed: %s", stage, count, r.errstr ? r.errstr(nr) : "?");
    }
    XV_CHECK_HIP(hipEventRecord(e->ev_comm, (hipStream_t)comm_stream));
    e->comm_pending = true;
    return 0;
}

extern "C" int xv_engine_allreduce_wait(xv_engine* e, void* stream) {
    XV_REQUIRE(e, "engine_allreduce_wait: null engine");
    if (e->comm_pending) {
        XV_CHECK_HIP(hipStreamWaitEvent((hipStream_t)stream, e->ev_comm, 0));
        e->comm_pending = false;
    }
    return 0;
}

extern "C" int xv_engine_stage_grad_range(const xv_engine* e, int stage, size_t* begin, size_t* end) {
    XV_REQUIRE(e && stage >= 0 && stage < XV_BWD_STAGES && begin && end, "stage_grad_range: bad arguments");
    *begin = e->stage_begin[stage];
    *end = e->stage_end[stage];
    return 0;
}

extern "C" int xv_engine_apply(xv_engine* e, void* stream, float lr, float grad_scale, int t) {
    XV_REQUIRE(e && e->V && e->G, "engine_apply: buffers not bound");
    XV_REQUIRE(e->cfg.optimizer == 0 || e->S, "engine_apply: optimiser state buffer not bound");
    hipStream_t s = (hipStream_t)stream;
    const xv_config& c = e->cfg;
    {   // the update rewrites the variables the side-stream halves of ensure_weights read (no-ops after a full step)
        int rcw = xve_wait_prep(e, s);
        if (rcw) return rcw;
        rcw = xve_wait_lossprep(e, s);
        if (rcw) return rcw;
    }
    if (c.clip_gradient_norm > 0.f) {
        XV_CHECK_HIP(hipMemsetAsync(e->scalars + 2, 0, sizeof(float), s));
        XV_REQUIRE(e->ws_bytes >= XV_SUMSQ_PARTS * sizeof(float), "engine_apply: workspace too small for the gradient norm");
        int rc = xv_sumsq_ordered(s, e->G, e->n_train, 1.0f, e->scalars + 2, (float*)e->ws);      // fixed order: the same bits on every rank and run
        if (rc) return rc;
        rc = xv_clip_scale(s, e->G, e->n_train, e->scalars + 2, grad_scale, c.clip_gradient_norm);
        if (rc) return rc;
        grad_scale = 1.0f;
    }
    int rc;
    if (c.optimizer == 0) rc = xv_sgd_update(s, e->V, e->G, e->n_train, lr, grad_scale);
    else if (c.optimizer == 1) rc = xv_momentum_update(s, e->V, e->G, e->S, e->n_train, lr, c.momentum, c.use_nesterov, grad_scale);
    else rc = xv_adam_update(s, e->V, e->G, e->S, e->S + e->n_train, e->n_train, lr, 0.9f, 0.999f, 1e-8f, t, grad_scale);
    e->weights_dirty = true;
    e->reg_valid = false;
    return rc;
}

extern "C" int xv_engine_loss_ptrs(xv_engine* e, float** raw_loss, float** reg_loss) {
    XV_REQUIRE(e && e->V, "loss_ptrs: engine not bound");
    if (reg_loss && !e->reg_valid) {
        int rc = xve_reg_loss(e, e->last_stream);
        if (rc) return rc;
    }
    if (raw_loss) *raw_loss = e->scalars + 0;
    if (reg_loss) *reg_loss = e->scalars + 1;
    return 0;
}

extern "C" int xv_debug_engine_clip_sumsq(xv_engine* e, float** sumsq) {
    XV_REQUIRE(e && e->scalars && sumsq, "debug_engine_clip_sumsq: engine not created");
    *sumsq = e->scalars + 2;
    return 0;
}

// (grows only; the stream is drained before a smaller buffer is freed: a copy of the previous endpoint may still be reading it)
float* xve_endpoint_scratch(xv_engine* e, size_t floats) {
    if (floats <= e->ep_scratch_floats) return e->ep_scratch;
    if (e->ep_scratch) {
        if (hipStreamSynchronize(e->last_stream) != hipSuccess) { xv_set_error("engine_endpoint: stream synchronisation failed"); return nullptr; }
        (void)hipFree(e->ep_scratch);
        e->ep_scratch = nullptr; e->ep_scratch_floats = 0;
    }
    if (hipMalloc((void**)&e->ep_scratch, floats * sizeof(float)) != hipSuccess) {
        xv_set_error("engine_endpoint: cannot allocate %zu bytes of endpoint scratch", floats * sizeof(float));
        return nullptr;
    }
    e->ep_scratch_floats = floats;
    return e->ep_scratch;
}

extern "C" int xv_engine_endpoint(xv_engine* e, const char* name, float** ptr, int32_t* rows, int32_t* cols, int32_t* ld) {
    XV_REQUIRE(e && name && ptr && rows && cols && ld, "engine_endpoint: null argument");
    XV_REQUIRE(e->B > 0, "engine_endpoint: run forward first");
    std::string n(name);
    const XvView view = {ptr, rows, cols, ld};
    for (int i = 0; i < e->NL; ++i) {
        XvAffine& a = e->L[i];
        if (n == a.prefix + "_" + a.kind) return view.set(a.z, a.rows, a.c_out, a.ldz);
        if (n == a.prefix + "_relu" && a.has_relu) {
            if ((e->f16 && (i < e->F - 1 || i == e->K0())) || i == e->F - 1) {     // not materialised on the hot path (fp16 planes / fused into pooling): rebuild on demand
                ActScope act(e, a);
                int rc = xv_bn_apply(e->last_stream, a.z, a.rows, a.c_out, a.ldz, a.scale, a.shift, 1, a.a, a.c_out);
                if (rc) return rc;
            }
            return view.set(i == e->S1() ? e->h7 : a.a, a.rows, a.c_out, a.c_out);
        }
        if (n == a.prefix + "_bn" && a.has_bn) {
            if (!a.has_relu) return view.set(i == e->S1() ? e->h7 : a.a, a.rows, a.c_out, a.c_out);
            // BN output is never materialised on the hot path (fused with ReLU): rebuild on demand
            float* sc = xve_endpoint_scratch(e, (size_t)a.rows * a.c_out);
            if (!sc) return 1;
            int rc = xv_bn_apply(e->last_stream, a.z, a.rows, a.c_out, a.ldz, a.scale, a.shift, 0, sc, a.c_out);
            if (rc) return rc;
            return view.set(sc, a.rows, a.c_out, a.c_out);
        }
    }
    int rc = xvp_endpoint(e, n, view);      // the pooling layer's views, then the loss head's
    if (rc != XV_EP_UNKNOWN) return rc;
    rc = xvh_endpoint(e, n, view);
    if (rc != XV_EP_UNKNOWN) return rc;
    if (n == "output") return view.set(e->out, e->B, e->Lout, e->Lout);
    xv_set_error("engine_endpoint: unknown endpoint '%s'", name);
    return XV_EP_UNKNOWN;
}
