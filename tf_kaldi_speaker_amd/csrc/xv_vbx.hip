// VB-HMM clustering of x-vectors (VBx, Landini et al.: the Bayesian HMM whose states are speakers, behind the agglomerative clusterer of
// xv_ahc.hip), as recalled from BUT's VB_diarization.py - nothing is compared with a run of that code.  One workgroup of 256 threads per
// recording, every iteration in one launch, the recordings of a call side by side.  Synchronisation is __syncthreads only - no grid-wide
// barrier, no wait on another workgroup, no atomics - so one recording cannot stall another, and a result depends on the recording's own
// inputs alone: every sum runs in a fixed order, the same bits every time.  gfx950 only.
//
// include/xvector_hip.h states the arithmetic; tests/vbx_ref.py restates it (the log-domain definition and the scaled form below).
//
// An iteration, for a recording of T rows, S speakers, D dimensions.  The speaker models and the scores are computed in DOUBLE from the
// fp32 inputs, the recursions in fp32: a score is a difference of sums of some hundred, and in fp32 its rounding alone (1e-5 of a nat)
// moves pi by a few 1e-6 - the float32 NumPy restatement shows as much, from one seed to the next between 1e-7 and 8e-6 - while the
// recursions, normalised per frame, lose a few ulps.  With one wave per SIMD a v_fma_f64 issues as often as a v_fma_f32, so the price is
// the conversions.  rho = X sqrt(Phi) is never formed: sqrt(Phi_d) is folded into the sums on either side.
//   (1) N_s = sum_t gamma_ts: thread (s, c) sums the rows t = c mod 8, the eight partials are added in ascending c.
//       sum_t gamma_ts X_td: P = the power of two >= D; thread (d, g) of 256 / P groups sums the rows t = g mod (256 / P) for eight
//       speakers at a time in registers (coalesced reads of X along d, gamma's row the same address in the whole group), the partials
//       go through the workspace and are added in ascending g.
//   (2) sixteen speakers at a time (LDS: 16 x 256 doubles), the thread of column d walks s: invL_sd = 1 / (1 + (fa / fb) N_s Phi_d),
//       alpha_sd = (fa / fb) invL_sd sqrt(Phi_d) sum_t gamma_ts X_td, and sqrt(Phi_d) alpha_sd goes into LDS; invL is consumed where it is
//       made - the row constant c_s = sum_d (invL + alpha^2) Phi_d and the ELBO's second term - so only alpha is kept; c_s by a butterfly per
//       wave and the waves in ascending order.
//   (3) scores' = fa (sum_d X_td sqrt(Phi_d) alpha_sd - c_s / 2) into the workspace, in double: a thread owns a row and eight speakers (a
//       wave: 64 rows, one group of speakers - alpha is a broadcast read of LDS, two columns a read; X a dword per lane whose cache line the
//       lane walks to its end).  fa G_t is the same for every speaker of a frame and is left out: it enters the log-likelihood only.
//   (4) per row: m_t = the largest score' among the live speakers (pi > 0), rounded to fp32 once; b_tj = exp(score'_tj - m_t) in fp32, the
//       difference taken in double; 0 for a dead speaker.
//   (5) forward, wave 0, speaker j in lane j: a_tj = b_tj (loop a^_{t-1,j} + (1 - loop) pi_j), n_t = sum_j a_tj, a^_t = a_t (1 / n_t).
//       The sum over the lanes is four DPP row rotations and two lane reads, the value of lane 0 and lane 16 for everybody - one instruction
//       stream, no LDS on the chain.  Loads run eight frames ahead of the chain.
//   (6) tll = sum_t (ln n_t + m_t) + fa sum_t G_t in double (a thread its rows, butterfly, waves in order).
//   (7) backward, wave 0: w = b_{t+1} * beta^_{t+1}, beta^_t = (loop w + (1 - loop) sum_j pi_j w_j) (1 / n_{t+1}), gamma_t = a^_t * beta^_t,
//       and the prior's sum acc_j += w_j (1 / n_{t+1}) in descending t;  pi_j = gamma_0j + (1 - loop) pi_j acc_j, then divided by its sum.
// The state between two iterations is (gamma, pi) in fp32 and nothing else: k iterations in one call are bit-equal to k calls of one.
//
// Out-of-range values (NaN inputs, a pi that is all zero) are undefined behaviour of the operation; they are not checked.
#include "xv_common.h"
#include "xv_ew.h"

#define VBX_MAX_T 2048
#define VBX_MAX_S 32
#define VBX_MAX_D 256
#define VBX_MAX_ITERS 64
#define VBX_THREADS 256
#define VBX_WAVES (VBX_THREADS / XV_WAVE)
#define VBX_SG 8            // speakers a thread accumulates at a time
#define VBX_HALF 16         // speakers whose models sit in LDS at a time
#define VBX_AHEAD 8         // frames whose loads are issued ahead of the recursions' chain (stores count in vmcnt too: a wait for loads drains them)

template <int CTRL>
__device__ __forceinline__ float vbx_dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// the sum of lanes 0 .. 31 of the wave, the same bits in every lane: each row of 16 lanes is summed by rotations (lane 0 of a row then
// holds one fixed tree over its row), and the two rows' lane-0 values are added, row 0 first
__device__ __forceinline__ float vbx_sum32(float v) {
    v += vbx_dpp<0x128>(v);      // row_ror:8
    v += vbx_dpp<0x124>(v);      // row_ror:4
    v += vbx_dpp<0x122>(v);      // row_ror:2
    v += vbx_dpp<0x121>(v);      // row_ror:1
    const float lo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float hi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    return lo + hi;
}

struct VbxArgs {
    const float* x; long x_floats;
    const int64_t* x_offsets; const int32_t* t; const int32_t* ld; const int32_t* s;
    int d; long total_t, total_ts, total_s;
    const float* phi; const float* gamma_in; const float* pi_in;
    float loop_prob, fa, fb; int max_iters; double epsilon;
    float* gamma; float* pi; double* elbo; int32_t* n_iters; int32_t* labels;
    float* ws;
};

// the workspace, in floats; the doubles of every recording first, so that they are 8-byte aligned: scores' [T][S] doubles, then the partial
// sums of the models [256][S] doubles, then per recording b [T][S], a^ [T][S], n [T], m [T]
static inline size_t vbx_ws_floats(long total_t, long total_ts, long total_s) {
    return 4 * (size_t)total_ts + 2 * (size_t)VBX_THREADS * (size_t)total_s + 2 * (size_t)total_t;
}

__global__ __launch_bounds__(VBX_THREADS) void vbx_kernel(VbxArgs g) {
    XV_EW_PRIORITY();
    __shared__ __attribute__((aligned(16))) double alpha[VBX_HALF * VBX_MAX_D];      // sqrt(Phi_d) alpha_sd of sixteen speakers, pitch D rounded up to 2
    __shared__ double npart[8][VBX_MAX_S];
    __shared__ double cpart[VBX_WAVES][VBX_MAX_S];
    __shared__ double n_s[VBX_MAX_S], c_s[VBX_MAX_S];
    __shared__ float pi_s[VBX_MAX_S];
    __shared__ double dred[VBX_WAVES];
    __shared__ long red[3][VBX_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), w = tid / XV_WAVE;

    // where this recording's rows, responsibilities and priors start: exclusive prefixes over the recordings before it, the counts
    // clamped into their ranges, and this recording's spans checked against the totals below - arrays the caller got wrong (it guarantees
    // them, ops.vbx checks them) cannot take a store outside the buffers of the call
    long pt = 0, pts = 0, ps = 0;
    for (int i = tid; i < r; i += VBX_THREADS) {
        const long ti = min(max(g.t[i], 1), VBX_MAX_T), si = min(max(g.s[i], 1), VBX_MAX_S);
        pt += ti;
        pts += ti * si;
        ps += si;
    }
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) {
        pt += __shfl_xor(pt, off);
        pts += __shfl_xor(pts, off);
        ps += __shfl_xor(ps, off);
    }
    if (lane == 0) { red[0][w] = pt; red[1][w] = pts; red[2][w] = ps; }
    __syncthreads();
    pt = pts = ps = 0;
#pragma unroll
    for (int i = 0; i < VBX_WAVES; ++i) { pt += red[0][i]; pts += red[1][i]; ps += red[2][i]; }
    const int T = g.t[r], S = g.s[r], ld = g.ld[r], D = g.d;
    const long x0 = g.x_offsets[r];
    if (T < 1 || T > VBX_MAX_T || S < 1 || S > VBX_MAX_S || ld < D || pt + T > g.total_t || pts + (long)T * S > g.total_ts ||
        ps + S > g.total_s || x0 < 0 || x0 + (long)(T - 1) * ld + D > g.x_floats) {
        if (tid == 0) g.n_iters[r] = -1;
        return;
    }
    const float* __restrict__ X = g.x + x0;
    double* score = (double*)g.ws + pts;                                                  // [T][S]
    double* part = (double*)g.ws + g.total_ts + (long)VBX_THREADS * ps;                   // [groups][S][P], groups * P = 256
    float* own = g.ws + 2 * g.total_ts + 2 * (long)VBX_THREADS * g.total_s + 2 * pts + 2 * pt;
    float* B = own;                          // b [T][S]
    float* ahat = B + (long)T * S;           // [T][S]
    float* nn = ahat + (long)T * S;          // [T]
    float* mx = nn + T;                      // [T]
    float* gam = g.gamma + pts;
    int32_t* labels = g.labels + pt;
    double* elbo = g.elbo + (long)r * g.max_iters;

    int P = 1;      // the power of two >= D
    while (P < D) P <<= 1;
    const int groups = VBX_THREADS / P, col = tid & (P - 1), grp = tid / P;
    const int de = (D + 1) & ~1;                                          // alpha's pitch in LDS: two columns a read
    const double phi_d = tid < D ? (double)g.phi[tid] : 0.0;              // column tid of the model
    const double root_d = sqrt(phi_d);
    const double c = (double)g.fa / (double)g.fb;
    const float lp = g.loop_prob, om = 1.f - g.loop_prob;

    // once per call: fa sum_t G_t, the state (gamma into the output, pi into LDS)
    double gsum = 0.0;
    for (int t = tid; t < T; t += VBX_THREADS) {
        double q = 0.0;
        for (int k = 0; k < D; ++k) {
            const double v = (double)X[(long)t * ld + k];
            q += v * v;
        }
        gsum += -0.5 * (q + (double)D * 1.8378770664093454835606594728112);
    }
    gsum = wave_sum(gsum);
    if (lane == 0) dred[w] = gsum;
    for (long i = tid; i < (long)T * S; i += VBX_THREADS) gam[i] = g.gamma_in[pts + i];
    if (tid < VBX_MAX_S) pi_s[tid] = tid < S ? g.pi_in[ps + tid] : 0.f;
    __syncthreads();
    gsum = (double)g.fa * (((dred[0] + dred[1]) + dred[2]) + dred[3]);
    __syncthreads();      // (dred is used again below)

    double prev = 0.0;
    int it = 0;
    for (; it < g.max_iters; ++it) {
        // (1) N_s and the partial sums of gamma^T X
        {
            const int s = tid & (VBX_MAX_S - 1), cth = tid / VBX_MAX_S;
            double acc = 0.0;
            if (s < S) {
#pragma unroll 8
                for (int t = cth; t < T; t += 8) acc += (double)gam[(long)t * S + s];
            }
            npart[cth][s] = acc;
        }
        for (int s0 = 0; s0 < S; s0 += VBX_SG) {
            double acc[VBX_SG];
#pragma unroll
            for (int u = 0; u < VBX_SG; ++u) acc[u] = 0.0;
            if (col < D) {
#pragma unroll 4
                for (int t = grp; t < T; t += groups) {      // (unrolled for loads in flight; an accumulator's adds keep their order)
                    const double x = (double)X[(long)t * ld + col];
                    const float* grow = gam + (long)t * S + s0;
#pragma unroll
                    for (int u = 0; u < VBX_SG; ++u) acc[u] = fma(s0 + u < S ? (double)grow[u] : 0.0, x, acc[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < VBX_SG; ++u)
                if (s0 + u < S) part[((long)grp * S + s0 + u) * P + col] = acc[u];
        }
        __syncthreads();
        if (tid < VBX_MAX_S) {
            double acc = npart[0][tid];
#pragma unroll
            for (int i = 1; i < 8; ++i) acc += npart[i][tid];
            n_s[tid] = acc;
        }
        __syncthreads();
        double e2 = 0.0;
        for (int sb = 0; sb < S; sb += VBX_HALF) {
            // (2) the models of sixteen speakers: column tid
            const int s_end = min(S, sb + VBX_HALF), s_pad = (s_end - sb + VBX_SG - 1) / VBX_SG * VBX_SG;
            for (int s = sb; s < sb + s_pad; ++s) {      // (the rows up to a multiple of eight are read below: zero)
                double term = 0.0, a_lds = 0.0;
                if (tid < D && s < s_end) {
                    double f = part[(long)s * P + tid];
                    for (int q = 1; q < groups; ++q) f += part[((long)q * S + s) * P + tid];
                    const double inv_l = 1.0 / (1.0 + c * n_s[s] * phi_d);
                    const double a = c * inv_l * (root_d * f);
                    a_lds = root_d * a;
                    term = (inv_l + a * a) * phi_d;
                    e2 += (log(inv_l) - inv_l - a * a) + 1.0;
                }
                if (tid < de) alpha[(s - sb) * de + tid] = a_lds;
                if (s < s_end) {      // (uniform)
                    term = wave_sum(term);
                    if (lane == 0) cpart[w][s] = term;
                }
            }
            __syncthreads();
            if (tid >= sb && tid < s_end) c_s[tid] = ((cpart[0][tid] + cpart[1][tid]) + cpart[2][tid]) + cpart[3][tid];
            __syncthreads();
            // (3) scores' = fa (X (sqrt(Phi) alpha)^T - c_s / 2): rows x groups of eight speakers
            {
                const int sgroups = s_pad / VBX_SG, rows = VBX_THREADS / sgroups;      // 1 or 2 groups: a wave holds one
                const int row = tid % rows, s0 = (tid / rows) * VBX_SG;
                for (int t = row; t < T; t += rows) {
                    double acc[VBX_SG];
#pragma unroll
                    for (int u = 0; u < VBX_SG; ++u) acc[u] = 0.0;
                    const float* xr = X + (long)t * ld;
#pragma unroll 4
                    for (int k = 0; k < de; k += 2) {
                        const double x0d = (double)xr[k], x1d = k + 1 < D ? (double)xr[k + 1] : 0.0;
#pragma unroll
                        for (int u = 0; u < VBX_SG; ++u) {
                            const double2 a = *(const double2*)(alpha + (s0 + u) * de + k);
                            acc[u] = fma(x1d, a.y, fma(x0d, a.x, acc[u]));
                        }
                    }
#pragma unroll
                    for (int u = 0; u < VBX_SG; ++u)
                        if (sb + s0 + u < S) score[(long)t * S + sb + s0 + u] = (double)g.fa * (acc[u] - 0.5 * c_s[sb + s0 + u]);
                }
            }
            __syncthreads();      // (alpha is written again by the next sixteen)
        }
        e2 = wave_sum(e2);
        if (lane == 0) dred[w] = e2;
        __syncthreads();
        const double second = 0.5 * (double)g.fb * (((dred[0] + dred[1]) + dred[2]) + dred[3]);
        // (4) per row: the largest score' among the live speakers, b
        for (int t = tid; t < T; t += VBX_THREADS) {
            const double* srow = score + (long)t * S;
            double m = -INFINITY;
            for (int s = 0; s < S; ++s)
                if (pi_s[s] > 0.f) m = fmax(m, srow[s]);
            const float mf = (float)m;
            for (int s = 0; s < S; ++s) B[(long)t * S + s] = pi_s[s] > 0.f ? expf((float)(srow[s] - (double)mf)) : 0.f;
            mx[t] = mf;
        }
        __syncthreads();
        // (5) forward
        const bool on = lane < S;
        const float pj = w == 0 && on ? pi_s[lane] : 0.f, ompj = om * pj;
        if (w == 0) {
            float ah = 0.f;
            for (int t0 = 0; t0 < T; t0 += VBX_AHEAD) {
                float bt[VBX_AHEAD];
#pragma unroll
                for (int u = 0; u < VBX_AHEAD; ++u) bt[u] = on && t0 + u < T ? B[(long)(t0 + u) * S + lane] : 0.f;
#pragma unroll
                for (int u = 0; u < VBX_AHEAD; ++u) {
                    const int t = t0 + u;
                    if (t < T) {      // (uniform)
                        const float a = bt[u] * (t == 0 ? pj : fmaf(lp, ah, ompj));
                        const float n = vbx_sum32(a);
                        ah = a * (1.f / n);
                        if (on) ahat[(long)t * S + lane] = ah;
                        if (lane == 0) nn[t] = n;
                    }
                }
            }
        }
        __syncthreads();
        // (6) the log-likelihood
        double tll = 0.0;
        for (int t = tid; t < T; t += VBX_THREADS) tll += log((double)nn[t]) + (double)mx[t];
        tll = wave_sum(tll);
        if (lane == 0) dred[w] = tll;
        // (7) backward and the priors
        if (w == 0) {
            float beta = 1.f, acc = 0.f;
            if (on) gam[(long)(T - 1) * S + lane] = ahat[(long)(T - 1) * S + lane];
            for (int t0 = T - 2; t0 >= 0; t0 -= VBX_AHEAD) {
                float bt[VBX_AHEAD], at[VBX_AHEAD], nt[VBX_AHEAD];
#pragma unroll
                for (int u = 0; u < VBX_AHEAD; ++u) {
                    const int t = t0 - u;
                    bt[u] = on && t >= 0 ? B[(long)(t + 1) * S + lane] : 0.f;
                    at[u] = on && t >= 0 ? ahat[(long)t * S + lane] : 0.f;
                    nt[u] = t >= 0 ? 1.f / nn[t + 1] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < VBX_AHEAD; ++u) {
                    const int t = t0 - u;
                    if (t >= 0) {      // (uniform)
                        const float wv = bt[u] * beta;
                        acc = fmaf(wv, nt[u], acc);
                        const float sw = vbx_sum32(pj * wv);
                        beta = fmaf(lp, wv, om * sw) * nt[u];
                        if (on) gam[(long)t * S + lane] = at[u] * beta;
                    }
                }
            }
            // (gamma's row 0 as it was just stored: T = 1 -> a^_0, else a^_0 * beta^_0 - recomputed, not re-read)
            const float g0 = T == 1 ? (on ? ahat[lane] : 0.f) : (on ? ahat[lane] * beta : 0.f);
            const float pn = on ? fmaf(ompj, acc, g0) : 0.f;
            const float total = vbx_sum32(pn);
            if (lane < VBX_MAX_S) pi_s[lane] = pn / total;
        }
        __syncthreads();
        const double e = ((((dred[0] + dred[1]) + dred[2]) + dred[3]) + gsum) + second;
        if (tid == 0) elbo[it] = e;
        __syncthreads();      // (dred and the state are read by everybody before the next iteration writes them)
        if (it > 0 && e - prev < g.epsilon) { ++it; break; }      // uniform: every thread holds the same e
        prev = e;
    }
    if (tid == 0) g.n_iters[r] = it;
    if (tid < S) g.pi[ps + tid] = pi_s[tid];
    for (int t = tid; t < T; t += VBX_THREADS) {
        const float* grow = gam + (long)t * S;
        float best = grow[0];
        int arg = 0;
        for (int s = 1; s < S; ++s)
            if (grow[s] > best) { best = grow[s]; arg = s; }
        labels[t] = arg;
    }
}

extern "C" size_t xv_vbx_workspace_bytes(int64_t total_t, int64_t total_ts, int64_t total_s, int d) {
    if (total_t <= 0 || total_ts <= 0 || total_s <= 0 || d <= 0) return 0;
    return vbx_ws_floats((long)total_t, (long)total_ts, (long)total_s) * sizeof(float);
}

extern "C" int xv_vbx(void* stream, const float* x, int64_t x_floats, const int64_t* x_offsets, const int32_t* t, const int32_t* ld,
                      const int32_t* s, int b, int d, int max_t, int max_s, int64_t total_t, int64_t total_ts, int64_t total_s,
                      const float* phi, const float* gamma_in, const float* pi_in, float loop_prob, float fa, float fb, int max_iters,
                      double epsilon, float* gamma, float* pi, double* elbo, int32_t* n_iters, int32_t* labels, void* ws, size_t ws_bytes) {
    XV_REQUIRE(b > 0, "vbx: no recording in the call (b=%d)", b);
    XV_REQUIRE(max_t >= 1 && max_s >= 1, "vbx: a recording needs at least one row and one speaker (largest T=%d, S=%d)", max_t, max_s);
    XV_REQUIRE(max_t <= VBX_MAX_T, "vbx: a recording of %d rows exceeds the cap of %d", max_t, VBX_MAX_T);
    XV_REQUIRE(max_s <= VBX_MAX_S, "vbx: %d speakers exceed the cap of %d", max_s, VBX_MAX_S);
    XV_REQUIRE(d >= 1 && d <= VBX_MAX_D, "vbx: d must lie in 1 .. %d (got %d)", VBX_MAX_D, d);
    XV_REQUIRE(max_iters >= 1 && max_iters <= VBX_MAX_ITERS, "vbx: max_iters must lie in 1 .. %d (got %d)", VBX_MAX_ITERS, max_iters);
    XV_REQUIRE(loop_prob > 0.f && loop_prob < 1.f, "vbx: loop_prob must lie strictly between 0 and 1 (got %g)", (double)loop_prob);
    XV_REQUIRE(fa > 0.f && fb > 0.f, "vbx: fa and fb must be positive (got %g, %g)", (double)fa, (double)fb);
    XV_REQUIRE(!(epsilon != epsilon), "vbx: epsilon is not a number");
    XV_REQUIRE(x && x_offsets && t && ld && s && phi && gamma_in && pi_in && gamma && pi && elbo && n_iters && labels && x_floats > 0,
               "vbx: bad arguments");
    XV_REQUIRE(total_t >= b && total_t <= (int64_t)b * max_t && total_s >= b && total_s <= (int64_t)b * max_s && total_ts >= total_t &&
               total_ts >= total_s && total_ts <= total_t * max_s,
               "vbx: total_t / total_ts / total_s do not fit b recordings of at most %d rows and %d speakers", max_t, max_s);
    const size_t need = vbx_ws_floats((long)total_t, (long)total_ts, (long)total_s) * sizeof(float);
    XV_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "vbx: workspace of %zu bytes, %zu needed, 16-byte aligned", ws_bytes, need);
    VbxArgs g;
    g.x = x; g.x_floats = (long)x_floats;
    g.x_offsets = x_offsets; g.t = t; g.ld = ld; g.s = s;
    g.d = d; g.total_t = (long)total_t; g.total_ts = (long)total_ts; g.total_s = (long)total_s;
    g.phi = phi; g.gamma_in = gamma_in; g.pi_in = pi_in;
    g.loop_prob = loop_prob; g.fa = fa; g.fb = fb; g.max_iters = max_iters; g.epsilon = epsilon;
    g.gamma = gamma; g.pi = pi; g.elbo = elbo; g.n_iters = n_iters; g.labels = labels;
    g.ws = (float*)ws;
    hipLaunchKernelGGL(vbx_kernel, dim3(b), dim3(VBX_THREADS), 0, (hipStream_t)stream, g);
    XV_LAUNCH_CHECK();
    return 0;
}
