// Agglomerative clustering of score matrices (speaker diarization: Kaldi's agglomerative-cluster behind ivector-plda-scoring-dense, as
// callhome_diarization/v2 runs it): average linkage on scores, one workgroup per recording, the recordings of a call side by side.
// Synchronisation is __syncthreads only - no grid-wide barrier, no wait on another workgroup, no atomics - so one recording cannot
// stall another, and a result depends on the recording's matrix alone: the same bits every time.  gfx950 only.
//
// The arithmetic is fixed to the operation (include/xvector_hip.h states it; tests/ahc_ref.py restates it in NumPy and the GPU's merge
// log is bit-equal to that at float32):
//     T[i][j] = T[j][i] = s[min(i,j)][max(i,j)];   A(a, b) = T[a][b] / (float)(size_a * size_b)        one IEEE fp32 divide
//     step:  the largest A over active pairs a < b, ties to the lowest a, then the lowest b
//     merge: T[a][k] = T[k][a] = T[a][k] + T[b][k] for every other active k (one fp32 add), size_a += size_b, b leaves
// (From singletons size_a * size_b <= 1024^2 < 2^24 is exact in fp32.  From a seed - xv_ahc_cluster_from, below - the sizes of a recording
// add up to at most 32768, so the int32 product is at most 2^28: it is exact as an integer and converted to fp32 once, round to nearest
// even, which is what (float)(sk * sc) does.)
//
// Long recordings (Kaldi's AgglomerativeClusterer::ClusterTwoPass, recalled and restated): xv_ahc_cluster_from clusters contiguous subsets
// down to a floor, xv_ahc_cluster_sums adds the scores between the surviving clusters into a seed, and xv_ahc_cluster_from, seeded, clusters
// the survivors - ops.ahc_cluster_two_pass drives the three.  DESIGN.md section 6l.
//
// State.  T lies in the workspace in full symmetric storage, pitch n, so that every read of the loop is a coalesced read along a row;
// the price is the n strided 4-byte stores of a merge (T[k][a]).  In LDS, for the cap of 2048 rows: size[] (0 = inactive), per row k
// the best pair of the row, bv[k] = max over active c > k of A(k, c) and bc[k] = its lowest column (-1: none), parent[] (the merge
// forest, read once at the end for the labels) and the repair lists - 40 KB of the 64 KB a workgroup gets by default.
//
// A step: (1) argmax over the n row bests (each thread its rows k = tid, tid + 256, ..., a butterfly per wave, four partials in LDS);
// (2) the row update: thread of column k adds T[b][k] into T[a][k] and T[k][a]; a row k < a whose best names neither a nor b compares
// the new A(k, a) with its best - nothing else in that row moved; a row k < b whose best named a or b goes on its wave's repair list
// (ballot + popcount: the list slot needs no atomic); (3) one wave per listed row, and one for row a, rescans that row of T.  Rows
// above b hold no pair with a or b and are not touched.
// Worst case of a step: n row bests, 2 n coalesced loads and n + n stores for the update, and (1 + r) row scans of at most n elements
// (one divide each), r = the rows below b whose best named a or b.  r < n, so an adversarial matrix (every row's best in one column) makes
// a step read n^2 / 2 elements; on scores of clustered embeddings r stays a handful, and a step is O(n) work behind four barriers.
// A recording takes at most n - 1 steps.  No rate is claimed here: profiles/ahc_bench.txt holds what was measured.
//
// A NaN score is undefined behaviour of the operation (every comparison with it is false); it is not checked.
#include "xv_common.h"
#include "xv_ew.h"

#define AHC_MAX_N 2048
#define AHC_MAX_POINTS 32768                    // the members of a seeded recording's clusters together; the rows xv_ahc_cluster_sums takes
#define AHC_THREADS 256
#define AHC_WAVES (AHC_THREADS / XV_WAVE)
#define AHC_COLS (AHC_MAX_N / AHC_THREADS)      // columns a thread owns at the cap
#define AHC_SCAN_UNROLL 4

// (v, i) beats (w, j): the larger value, on a tie the lower index; an index below 0 is "nothing yet"
__device__ __forceinline__ bool ahc_better(float v, int i, float w, int j) { return i >= 0 && (j < 0 || v > w || (v == w && i < j)); }

// the best (value, index) of the wave, in every lane: indices differ between lanes (or are < 0), so the order of the exchanges is immaterial
__device__ __forceinline__ void ahc_wave_best(float& v, int& i) {
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) {
        const float w = __shfl_xor(v, off);
        const int j = __shfl_xor(i, off);
        if (ahc_better(w, j, v, i)) { v = w; i = j; }
    }
}

// row k's best pair over the active columns c > k, by one wave; a lane walks its columns upwards, so `>` keeps the lowest on a tie
__device__ __forceinline__ void ahc_scan_row(const float* row, int k, int n, const int* size, float* bv, int* bc, int lane) {
    const int sk = size[k];
    float v = 0.f;
    int best = -1;
    // four loads in flight per lane, issued whatever the columns' activity (a load behind the test would wait out its latency alone)
    for (int c0 = k + 1 + lane; c0 < n; c0 += AHC_SCAN_UNROLL * XV_WAVE) {
        float t[AHC_SCAN_UNROLL];
#pragma unroll
        for (int u = 0; u < AHC_SCAN_UNROLL; ++u) {
            const int c = c0 + u * XV_WAVE;
            t[u] = c < n ? row[c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < AHC_SCAN_UNROLL; ++u) {
            const int c = c0 + u * XV_WAVE;
            const int sc = c < n ? size[c] : 0;
            if (sc > 0) {
                const float a = t[u] / (float)(sk * sc);
                if (best < 0 || a > v) { v = a; best = c; }
            }
        }
    }
    ahc_wave_best(v, best);
    if (lane == 0) { bv[k] = v; bc[k] = best; }
}

struct AhcArgs {
    const float* scores; long scores_floats;
    const int64_t* mat_offsets; const int32_t* n; const int32_t* ld; const int32_t* targets;
    long total_n; long sum_n2; float threshold;
    int32_t* labels; int32_t* merges; float* merge_values; int32_t* n_merges;
    float* ws;
};

struct AhcFromArgs : AhcArgs {
    const int32_t* sizes; int seeded;
};

// Both clusterers.  <false, AhcArgs> is xv_ahc_cluster: clusters start as singletons, targets[r] and the threshold stop the merging.
// <true, AhcFromArgs> is xv_ahc_cluster_from: g.targets holds the floors (merge while count > floor and A >= threshold); with g.seeded the
// clusters start from g.sizes and the T the caller left in the workspace, and the scores are not touched.  The first instantiation has
// the registers, LDS and code bytes the kernel had before the second existed (profiles/ahc_two_pass_registers.txt).
template <bool FROM, class Args>
__global__ __launch_bounds__(AHC_THREADS) void ahc_cluster_kernel(Args g) {
    bool seeded = false;
    const int32_t* seed_sizes = nullptr;
    if constexpr (FROM) { seeded = g.seeded != 0; seed_sizes = g.sizes; }
    XV_EW_PRIORITY();
    __shared__ int size[AHC_MAX_N];
    __shared__ float bv[AHC_MAX_N];
    __shared__ int bc[AHC_MAX_N];
    __shared__ int parent[AHC_MAX_N];
    __shared__ int list[AHC_WAVES][AHC_MAX_N / AHC_WAVES];
    __shared__ int lcount[AHC_WAVES];
    __shared__ float red_v[AHC_WAVES];
    __shared__ int red_i[AHC_WAVES];
    __shared__ long red_n[AHC_WAVES], red_t[AHC_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), w = tid / XV_WAVE;

    // where this recording's outputs and its T start: the exclusive prefixes of n and n^2 over the recordings before it.  (A count is
    // clamped into 1 .. the cap here and this recording's spans are checked against the totals below, so that even arrays the caller
    // got wrong - it guarantees them, ops.ahc_cluster checks them - cannot take a store outside the buffers of the call.)
    long pn = 0, pt = 0;
    for (int i = tid; i < r; i += AHC_THREADS) {
        const long ni = min(max(g.n[i], 1), AHC_MAX_N);
        pn += ni;
        pt += ni * ni;
    }
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) {
        pn += __shfl_xor(pn, off);
        pt += __shfl_xor(pt, off);
    }
    if (lane == 0) { red_n[w] = pn; red_t[w] = pt; }
    __syncthreads();
    pn = pt = 0;
#pragma unroll
    for (int i = 0; i < AHC_WAVES; ++i) { pn += red_n[i]; pt += red_t[i]; }
    const long pm = pn - r;      // the merges before this recording: sum of (n - 1)
    // (a seeded start has no scores: the entry point hands over n as ld and the workspace as scores, so that the checks hold as they stand)
    const int n = g.n[r], ld = g.ld[r], target = g.targets[r];
    const long s0 = seeded ? 0 : g.mat_offsets[r];
    if (n < 1 || n > AHC_MAX_N || ld < n || target < (FROM ? 1 : 0) || target > n || pn + n > g.total_n || pt + (long)n * n > g.sum_n2 || s0 < 0 ||
        s0 + (long)(n - 1) * ld + n > g.scores_floats) {
        if (tid == 0) g.n_merges[r] = -1;
        return;
    }
    const float* __restrict__ S = g.scores + s0;
    float* T = g.ws + pt;
    if (seeded) {
        // the seed: T is in place; the sizes are checked (each >= 1, together at most AHC_MAX_POINTS, so that no product of two leaves
        // int32) before anything depends on them - a size of 0 would be an inactive cluster without a parent
        long total = 0, bad = 0;
        for (int k = tid; k < n; k += AHC_THREADS) {
            const int sk = seed_sizes[pn + k];
            size[k] = sk;
            parent[k] = k;
            total += sk > 0 ? sk : 0;
            bad += sk < 1 ? 1 : 0;
        }
#pragma unroll
        for (int off = XV_WAVE / 2; off; off >>= 1) {
            total += __shfl_xor(total, off);
            bad += __shfl_xor(bad, off);
        }
        __syncthreads();      // every thread has read the prefixes out of red_n / red_t
        if (lane == 0) { red_n[w] = total; red_t[w] = bad; }
        __syncthreads();
        total = bad = 0;
#pragma unroll
        for (int i = 0; i < AHC_WAVES; ++i) { total += red_n[i]; bad += red_t[i]; }
        if (bad || total > AHC_MAX_POINTS) {      // (uniform)
            if (tid == 0) g.n_merges[r] = -1;
            return;
        }
    } else {
        // T from the upper triangle: row i of s is read along the row, T[i][j] stored along the row and T[j][i] down the column
        // (a thread's loads of a row are issued together, ahead of their stores: AHC_COLS in flight)
        for (int i = 0; i < n; ++i) {
            float t[AHC_COLS];
#pragma unroll
            for (int u = 0; u < AHC_COLS; ++u) {
                const int j = i + tid + u * AHC_THREADS;
                t[u] = j < n && j != i ? S[(long)i * ld + j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < AHC_COLS; ++u) {
                const int j = i + tid + u * AHC_THREADS;
                if (j < n) {
                    T[(long)i * n + j] = t[u];
                    T[(long)j * n + i] = t[u];
                }
            }
        }
        for (int k = tid; k < n; k += AHC_THREADS) { size[k] = 1; parent[k] = k; }
    }
    __syncthreads();
    for (int k = w; k < n; k += AHC_WAVES) ahc_scan_row(T + (long)k * n, k, n, size, bv, bc, lane);
    __syncthreads();

    const int stop_at = FROM || target > 1 ? target : 1;
    int count = n, nm = 0;
    while (count > stop_at) {
        // (1) the best pair: rows walked upwards by a thread, so its own ties go to the lowest row already
        float v = 0.f;
        int a = -1;
        for (int k = tid; k < n; k += AHC_THREADS)
            if (size[k] > 0 && bc[k] >= 0 && ahc_better(bv[k], k, v, a)) { v = bv[k]; a = k; }
        ahc_wave_best(v, a);
        if (lane == 0) { red_v[w] = v; red_i[w] = a; }
        __syncthreads();
        v = red_v[0]; a = red_i[0];
#pragma unroll
        for (int i = 1; i < AHC_WAVES; ++i)
            if (ahc_better(red_v[i], red_i[i], v, a)) { v = red_v[i]; a = red_i[i]; }
        if (a < 0) break;                                   // (cannot happen with count >= 2; uniform)
        if ((FROM || target == 0) && !(v >= g.threshold)) break;      // uniform: every thread holds the same (v, a)
        const int b = bc[a], sa = size[a], sb = size[b], sab = sa + sb;
        if (tid == 0) {
            g.merges[2 * (pm + nm)] = a;
            g.merges[2 * (pm + nm) + 1] = b;
            g.merge_values[pm + nm] = v;
        }
        ++nm;
        // (2) b into a
        float* Ta = T + (long)a * n;
        const float* Tb = T + (long)b * n;
        int cnt = 0;
        // both rows first, every column a thread owns in flight together; the adds and the stores follow
        float ra[AHC_COLS], rb[AHC_COLS];
#pragma unroll
        for (int u = 0; u < AHC_COLS; ++u) {
            const int k = u * AHC_THREADS + tid;
            ra[u] = k < n ? Ta[k] : 0.f;
            rb[u] = k < n ? Tb[k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < AHC_COLS; ++u) {
            if (u * AHC_THREADS >= n) break;      // (uniform: the ballot below is taken by whole waves)
            const int k = u * AHC_THREADS + tid;
            bool need = false;
            if (k < n && k != a && k != b) {
                const int sk = size[k];
                if (sk > 0) {
                    const float t = ra[u] + rb[u];
                    Ta[k] = t;
                    T[(long)k * n + a] = t;
                    if (k < b) {
                        const int c = bc[k];
                        if (c == a || c == b) {
                            need = true;
                        } else if (k < a) {
                            const float cand = t / (float)(sab * sk);
                            if (cand > bv[k] || (cand == bv[k] && a < c)) { bv[k] = cand; bc[k] = a; }
                        }
                    }
                }
            }
            const unsigned long long m = __ballot(need);
            if (need) list[w][cnt + __popcll(m & ((1ull << lane) - 1ull))] = k;
            cnt += __popcll(m);
        }
        if (lane == 0) lcount[w] = cnt;
        __syncthreads();      // every thread has read size[a], size[b]; T's row a and the lists are complete
        if (tid == 0) { size[a] = sab; size[b] = 0; bc[b] = -1; parent[b] = a; }
        __syncthreads();
        // (3) the rows whose best is gone, and row a
        int total = 0;
#pragma unroll
        for (int i = 0; i < AHC_WAVES; ++i) total += lcount[i];
        for (int i = w; i <= total; i += AHC_WAVES) {
            int k = a;
            if (i < total) {
                int q = i, l = 0;
                while (q >= lcount[l]) { q -= lcount[l]; ++l; }
                k = list[l][q];
            }
            ahc_scan_row(T + (long)k * n, k, n, size, bv, bc, lane);
        }
        __syncthreads();
        --count;
    }
    if (tid == 0) g.n_merges[r] = nm;
    // labels: a cluster's id is its smallest member - the root of the merge forest, since b > a always joins a; the final clusters are
    // numbered in ascending id
    for (int m = tid; m < n; m += AHC_THREADS) {
        int root = m;
        while (size[root] == 0) root = parent[root];
        int label = 0;
        for (int c = 0; c < root; ++c) label += size[c] > 0 ? 1 : 0;
        g.labels[pn + m] = label;
    }
}

// ---- cluster sums: the seed of a second pass (xv_ahc_cluster_sums; include/xvector_hip.h states the order of every sum, tests/ahc2_ref.py
// restates it).  Three launches in stream order, no atomics, no wait on another workgroup:
//   plan   one workgroup per recording: the exclusive prefixes (n, c, c^2, n c) that place its lists, outputs and scratch, and the checks
//          that keep every later access inside the buffers of the call (spans against the totals, starts ascending from 0 to n, members
//          in 0 .. n - 1); status[r] = 0, or -1 and the recording is skipped by the two kernels below
//   rows   R[i][B] = the sequential double sum over the members j of B, ascending, of e(i, j) = s[min(i,j)][max(i,j)] (0 for j = i).  A
//          wave takes 64 consecutive rows i and one cluster B: the member index is the same in every lane (scalar loads), for j below
//          the rows the lanes read s[j][i .. i + 63], one coalesced 256-byte read; for j above them lane l reads s[i + l][j], 64 cache
//          lines, which the following members of the cluster (first-pass clusters are mostly runs of consecutive windows) find in L1 / L2
//   fold   T[A][B] = T[B][A] = fp32(the sequential double sum over the members i of A, ascending, of R[i][B]) for A < B, a thread per
//          B and a workgroup per (A, 256 values of B): R[i][B .. B + 255] is read coalesced; the diagonal is 0; sizes[A] = |A|
// R is n x c doubles of scratch: each matrix element is read twice (once for either row), every R entry written and read once.
#define AHCS_THREADS 256
#define AHCS_ROWS XV_WAVE                          // rows of a workgroup of the rows kernel: a lane each
#define AHCS_CLUSTERS (AHCS_THREADS / XV_WAVE)     // ... and its clusters: a wave each
#define AHCS_UNROLL 4

struct AhcSumsArgs {
    const float* scores; long scores_floats;
    const int64_t* mat_offsets; const int32_t* n; const int32_t* ld; const int32_t* c;
    const int32_t* members; const int32_t* starts;
    long total_n, total_c, sum_c2, sum_nc;
    float* seed; int32_t* sizes; int32_t* status;
    double* rows; long* plan;      // the workspace: R of every recording, then [b][4] prefixes
};

__global__ __launch_bounds__(AHCS_THREADS) void ahc_sums_plan_kernel(AhcSumsArgs g) {
    __shared__ long red[4][AHCS_THREADS / XV_WAVE];
    __shared__ int any_bad;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), w = tid / XV_WAVE;
    long p[4] = {0, 0, 0, 0};
    for (int i = tid; i < r; i += AHCS_THREADS) {      // (counts clamped into their ranges, as in the clusterer)
        const long ni = min(max(g.n[i], 1), AHC_MAX_POINTS), ci = min(max(g.c[i], 1), AHC_MAX_N);
        p[0] += ni; p[1] += ci; p[2] += ci * ci; p[3] += ni * ci;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int off = XV_WAVE / 2; off; off >>= 1) p[q] += __shfl_xor(p[q], off);
        if (lane == 0) red[q][w] = p[q];
    }
    if (tid == 0) any_bad = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        p[q] = 0;
#pragma unroll
        for (int i = 0; i < AHCS_THREADS / XV_WAVE; ++i) p[q] += red[q][i];
    }
    const int n = g.n[r], c = g.c[r], ld = g.ld[r];
    const long s0 = g.mat_offsets[r];
    bool ok = n >= 1 && n <= AHC_MAX_POINTS && c >= 1 && c <= AHC_MAX_N && c <= n && ld >= n && p[0] + n <= g.total_n && p[1] + c <= g.total_c &&
              p[2] + (long)c * c <= g.sum_c2 && p[3] + (long)n * c <= g.sum_nc && s0 >= 0 && s0 + (long)(n - 1) * ld + n <= g.scores_floats;
    if (ok) {      // (uniform) the lists lie inside their buffers: their entries may be read
        const int32_t* st = g.starts + p[1] + r;
        const int32_t* mem = g.members + p[0];
        bool bad = false;
        for (int k = tid; k <= c; k += AHCS_THREADS) bad |= k == 0 ? st[0] != 0 : (st[k] <= st[k - 1] || (k == c && st[k] != n));
        for (int k = tid; k < n; k += AHCS_THREADS) bad |= mem[k] < 0 || mem[k] >= n;
        if (bad) any_bad = 1;      // (every writer stores the same value)
    }
    __syncthreads();
    if (tid == 0) {
        g.status[r] = ok && !any_bad ? 0 : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) g.plan[4 * r + q] = p[q];
    }
}

__global__ __launch_bounds__(AHCS_THREADS) void ahc_sums_rows_kernel(AhcSumsArgs g) {
    const int r = blockIdx.z;
    if (g.status[r] != 0) return;
    const int n = g.n[r], c = g.c[r], ld = g.ld[r];
    const int lane = threadIdx.x & (XV_WAVE - 1);
    const int B = blockIdx.y * AHCS_CLUSTERS + __builtin_amdgcn_readfirstlane(threadIdx.x / XV_WAVE);
    const int i0 = blockIdx.x * AHCS_ROWS, i = i0 + lane;
    if (B >= c || i0 >= n) return;      // (uniform in the wave; no barrier below)
    const long* P = g.plan + 4 * r;
    const float* __restrict__ S = g.scores + g.mat_offsets[r];
    const int32_t* __restrict__ mem = g.members + P[0];
    const int32_t* st = g.starts + P[1] + r;
    const int k0 = st[B], k1 = st[B + 1];
    if (i >= n) return;
    // e(i, j): the upper triangle only; a thread's loads of a round are issued together, the adds follow in the members' order
    auto e = [&](int j) { return j == i ? 0.f : (j < i ? S[(long)j * ld + i] : S[(long)i * ld + j]); };
    double acc = (double)e(mem[k0]);      // (the first member starts the sum: no 0.0 in front of it)
    int k = k0 + 1;
    for (; k + AHCS_UNROLL <= k1; k += AHCS_UNROLL) {
        float v[AHCS_UNROLL];
#pragma unroll
        for (int u = 0; u < AHCS_UNROLL; ++u) v[u] = e(mem[k + u]);
#pragma unroll
        for (int u = 0; u < AHCS_UNROLL; ++u) acc += (double)v[u];
    }
    for (; k < k1; ++k) acc += (double)e(mem[k]);
    g.rows[P[3] + (long)i * c + B] = acc;
}

__global__ __launch_bounds__(AHCS_THREADS) void ahc_sums_fold_kernel(AhcSumsArgs g) {
    const int r = blockIdx.z, A = blockIdx.y, B = blockIdx.x * AHCS_THREADS + threadIdx.x;
    if (g.status[r] != 0) return;
    const int c = g.c[r];
    if (A >= c || blockIdx.x * AHCS_THREADS + AHCS_THREADS - 1 < A) return;      // (uniform: nothing at or right of the diagonal here)
    const long* P = g.plan + 4 * r;
    const int32_t* __restrict__ mem = g.members + P[0];
    const int32_t* st = g.starts + P[1] + r;
    const int k0 = st[A], k1 = st[A + 1];
    float* T = g.seed + P[2];
    if (B >= c || B < A) return;
    if (B == A) {
        T[(long)A * c + A] = 0.f;
        g.sizes[P[1] + A] = k1 - k0;
        return;
    }
    const double* __restrict__ R = g.rows + P[3] + B;
    double acc = R[(long)mem[k0] * c];
    int k = k0 + 1;
    for (; k + AHCS_UNROLL <= k1; k += AHCS_UNROLL) {
        double v[AHCS_UNROLL];
#pragma unroll
        for (int u = 0; u < AHCS_UNROLL; ++u) v[u] = R[(long)mem[k + u] * c];
#pragma unroll
        for (int u = 0; u < AHCS_UNROLL; ++u) acc += v[u];
    }
    for (; k < k1; ++k) acc += R[(long)mem[k] * c];
    const float t = (float)acc;
    T[(long)A * c + B] = t;
    T[(long)B * c + A] = t;
}

// ---- labels at many cuts of one merge log (xv_ahc_cut; include/xvector_hip.h states the rule, tests/diar_eval_ref.py restates it).  A
// threshold changes the clusterer's stop rule and nothing else, so the log of a run down to one cluster holds the labels of every
// threshold as a prefix.  One workgroup per (recording, cut), no hand-over between workgroups, integers only behind the comparison of the
// logged values with the threshold: the same bits every time.
//   p      the first log entry that fails A >= threshold (a min over the failing entries: an fp32 log need not be monotone), then the two
//          clamps of the cut
//   forest parent[b] = a for the first p entries: independent 4-byte LDS stores, since a row leaves once.  An entry is taken only with
//          0 <= a < b < n, so that a log the caller got wrong can neither leave the arrays nor close a cycle (the walk below ends)
//   labels every row walks to its root (its cluster's smallest member); the roots are numbered by a prefix count: a ballot per wave and
//          AHC_COLS x AHC_WAVES wave totals, summed by one thread
__device__ __forceinline__ int ahc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct AhcCutArgs {
    const int32_t* merges; const float* merge_values; const int32_t* n_merges; const int32_t* n;
    const float* thresholds; const int32_t* min_clusters; const int32_t* max_clusters;
    int b; long total_n;
    int32_t* labels; int32_t* clusters;
};

__global__ __launch_bounds__(AHC_THREADS) void ahc_cut_kernel(AhcCutArgs g) {
    __shared__ int parent[AHC_MAX_N];
    __shared__ int rank[AHC_MAX_N];
    __shared__ int wave_roots[AHC_COLS * AHC_WAVES];
    __shared__ long red_n[AHC_WAVES];
    __shared__ int red_p[AHC_WAVES];
    __shared__ int any_bad;
    const int r = blockIdx.x, cut = blockIdx.y, tid = threadIdx.x, lane = tid & (XV_WAVE - 1), w = tid / XV_WAVE;
    long pn = 0;      // (the exclusive prefix of n, counts clamped as in the clusterer)
    for (int i = tid; i < r; i += AHC_THREADS) pn += min(max(g.n[i], 1), AHC_MAX_N);
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) pn += __shfl_xor(pn, off);
    if (lane == 0) red_n[w] = pn;
    if (tid == 0) any_bad = 0;
    __syncthreads();
    pn = 0;
#pragma unroll
    for (int i = 0; i < AHC_WAVES; ++i) pn += red_n[i];
    const long pm = pn - r;
    const int n = g.n[r], nm = g.n_merges[r];
    const float threshold = g.thresholds[cut];
    const int lo = g.min_clusters[cut], hi = g.max_clusters[cut];
    int32_t* count_out = g.clusters + (long)cut * g.b + r;
    // (uniform; the log's n - 1 slots must end inside the total_n - b of the call, as the labels inside total_n)
    if (n < 1 || n > AHC_MAX_N || nm < 0 || nm > n - 1 || pn + n > g.total_n || pm + n - 1 > g.total_n - g.b || lo < 1 || hi < lo || threshold != threshold) {
        if (tid == 0) *count_out = -1;
        return;
    }
    int p = nm;
    for (int i = tid; i < nm; i += AHC_THREADS)
        if (!(g.merge_values[pm + i] >= threshold)) { p = i; break; }      // (a thread's entries ascend: its first failing one)
#pragma unroll
    for (int off = XV_WAVE / 2; off; off >>= 1) p = min(p, __shfl_xor(p, off));
    if (lane == 0) red_p[w] = p;
    for (int k = tid; k < n; k += AHC_THREADS) parent[k] = k;
    __syncthreads();
    p = red_p[0];
#pragma unroll
    for (int i = 1; i < AHC_WAVES; ++i) p = min(p, red_p[i]);
    p = ahc_clamp(min(p, n - lo), 0, nm);
    p = ahc_clamp(max(p, n - hi), 0, nm);
    for (int i = tid; i < p; i += AHC_THREADS) {
        const int a = g.merges[2 * (pm + i)], c = g.merges[2 * (pm + i) + 1];
        if (a >= 0 && a < c && c < n) parent[c] = a;
        else any_bad = 1;      // (every writer stores the same value)
    }
    __syncthreads();
    if (any_bad) {      // (uniform)
        if (tid == 0) *count_out = -1;
        return;
    }
    int root[AHC_COLS];
#pragma unroll
    for (int u = 0; u < AHC_COLS; ++u) {
        if (u * AHC_THREADS >= n) break;      // (uniform: the ballot is taken by whole waves)
        const int k = u * AHC_THREADS + tid;
        int at = k < n ? k : 0;
        while (parent[at] != at) at = parent[at];
        root[u] = at;
        const unsigned long long m = __ballot(k < n && at == k);
        if (k < n) rank[k] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_roots[u * AHC_WAVES + w] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) {      // the exclusive prefix of the wave totals, the clusters of this cut behind it
        int sum = 0;
        for (int i = 0; i < AHC_COLS * AHC_WAVES && (i / AHC_WAVES) * AHC_THREADS < n; ++i) {
            const int c = wave_roots[i];
            wave_roots[i] = sum;
            sum += c;
        }
        *count_out = sum;
    }
    __syncthreads();
    int32_t* out = g.labels + (long)cut * g.total_n + pn;
#pragma unroll
    for (int u = 0; u < AHC_COLS; ++u) {
        if (u * AHC_THREADS >= n) break;
        const int k = u * AHC_THREADS + tid;
        // (a root's rank: its place among the roots of its wave's 64 rows, behind the roots of the waves before)
        if (k < n) out[k] = rank[root[u]] + wave_roots[(root[u] / AHC_THREADS) * AHC_WAVES + (root[u] % AHC_THREADS) / XV_WAVE];
    }
}

extern "C" size_t xv_ahc_workspace_bytes(int64_t sum_n2) { return (size_t)(sum_n2 > 0 ? sum_n2 : 0) * sizeof(float); }

extern "C" int xv_ahc_cluster(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n,
                              const int32_t* ld, const int32_t* targets, int b, int max_n, int64_t total_n, int64_t sum_n2, float threshold,
                              int32_t* labels, int32_t* merges, float* merge_values, int32_t* n_merges, void* ws, size_t ws_bytes) {
    XV_REQUIRE(b > 0, "ahc_cluster: no recording in the call (b=%d)", b);
    XV_REQUIRE(max_n >= 1, "ahc_cluster: a recording needs at least one row (largest n=%d)", max_n);
    XV_REQUIRE(max_n <= AHC_MAX_N, "ahc_cluster: a recording of %d rows exceeds the cap of %d", max_n, AHC_MAX_N);
    XV_REQUIRE(scores && mat_offsets && n && ld && targets && labels && n_merges && scores_floats > 0, "ahc_cluster: bad arguments");
    XV_REQUIRE(total_n >= b && total_n <= (int64_t)b * max_n && sum_n2 >= total_n && sum_n2 <= total_n * max_n,
               "ahc_cluster: total_n / sum_n2 do not fit b recordings of at most %d rows", max_n);
    XV_REQUIRE(total_n == b || (merges && merge_values), "ahc_cluster: merges and merge_values are needed (some recording has two rows or more)");
    XV_REQUIRE(ws && ws_bytes / sizeof(float) >= (size_t)sum_n2, "ahc_cluster: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)sum_n2 * sizeof(float));
    AhcArgs g;
    g.scores = scores; g.scores_floats = (long)scores_floats;
    g.mat_offsets = mat_offsets; g.n = n; g.ld = ld; g.targets = targets;
    g.total_n = (long)total_n; g.sum_n2 = (long)sum_n2; g.threshold = threshold;
    g.labels = labels; g.merges = merges; g.merge_values = merge_values; g.n_merges = n_merges;
    g.ws = (float*)ws;
    hipLaunchKernelGGL((ahc_cluster_kernel<false, AhcArgs>), dim3(b), dim3(AHC_THREADS), 0, (hipStream_t)stream, g);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t xv_ahc_cluster_from_workspace_bytes(int64_t sum_n2) { return xv_ahc_workspace_bytes(sum_n2); }

extern "C" int xv_ahc_cluster_from(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n,
                                   const int32_t* ld, const int32_t* floors, const int32_t* sizes, int seeded, int b, int max_n, int64_t total_n,
                                   int64_t sum_n2, float threshold, int32_t* labels, int32_t* merges, float* merge_values, int32_t* n_merges,
                                   void* ws, size_t ws_bytes) {
    XV_REQUIRE(b > 0, "ahc_cluster_from: no recording in the call (b=%d)", b);
    XV_REQUIRE(max_n >= 1, "ahc_cluster_from: a recording needs at least one row (largest n=%d)", max_n);
    XV_REQUIRE(max_n <= AHC_MAX_N, "ahc_cluster_from: a recording of %d rows exceeds the cap of %d", max_n, AHC_MAX_N);
    XV_REQUIRE(seeded == 0 || seeded == 1, "ahc_cluster_from: seeded must be 0 (start from the scores) or 1 (got %d)", seeded);
    XV_REQUIRE(threshold == threshold, "ahc_cluster_from: the threshold is NaN (-inf merges down to the floor)");
    XV_REQUIRE(n && floors && labels && n_merges, "ahc_cluster_from: bad arguments");
    XV_REQUIRE(seeded || (scores && mat_offsets && ld && scores_floats > 0), "ahc_cluster_from: a start from the scores needs scores, mat_offsets and ld");
    XV_REQUIRE(!seeded || sizes, "ahc_cluster_from: a seeded start needs the clusters' sizes");
    XV_REQUIRE(total_n >= b && total_n <= (int64_t)b * max_n && sum_n2 >= total_n && sum_n2 <= total_n * max_n,
               "ahc_cluster_from: total_n / sum_n2 do not fit b recordings of at most %d rows", max_n);
    XV_REQUIRE(total_n == b || (merges && merge_values), "ahc_cluster_from: merges and merge_values are needed (some recording has two rows or more)");
    XV_REQUIRE(ws && ws_bytes / sizeof(float) >= (size_t)sum_n2, "ahc_cluster_from: workspace of %zu bytes, %zu needed", ws_bytes,
               (size_t)sum_n2 * sizeof(float));
    AhcFromArgs g;
    g.sizes = sizes; g.seeded = seeded;
    g.scores = seeded ? (const float*)ws : scores; g.scores_floats = seeded ? (long)sum_n2 : (long)scores_floats;
    g.mat_offsets = mat_offsets; g.n = n; g.ld = seeded ? n : ld; g.targets = floors;
    g.total_n = (long)total_n; g.sum_n2 = (long)sum_n2; g.threshold = threshold;
    g.labels = labels; g.merges = merges; g.merge_values = merge_values; g.n_merges = n_merges;
    g.ws = (float*)ws;
    hipLaunchKernelGGL((ahc_cluster_kernel<true, AhcFromArgs>), dim3(b), dim3(AHC_THREADS), 0, (hipStream_t)stream, g);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t xv_ahc_cluster_sums_workspace_bytes(int b, int64_t sum_nc) {
    return (size_t)(sum_nc > 0 ? sum_nc : 0) * sizeof(double) + (size_t)(b > 0 ? b : 0) * 4 * sizeof(long);
}

extern "C" int xv_ahc_cluster_sums(void* stream, const float* scores, int64_t scores_floats, const int64_t* mat_offsets, const int32_t* n,
                                   const int32_t* ld, const int32_t* c, const int32_t* members, const int32_t* starts, int b, int max_n,
                                   int max_c, int64_t total_n, int64_t total_c, int64_t sum_c2, int64_t sum_nc, float* seed, int32_t* sizes,
                                   int32_t* status, void* ws, size_t ws_bytes) {
    XV_REQUIRE(b > 0 && b <= 65535, "ahc_cluster_sums: 1 .. 65535 recordings in a call (b=%d)", b);
    XV_REQUIRE(max_n >= 1 && max_c >= 1, "ahc_cluster_sums: a recording needs at least one row and one cluster (largest n=%d, c=%d)", max_n, max_c);
    XV_REQUIRE(max_n <= AHC_MAX_POINTS, "ahc_cluster_sums: a recording of %d rows exceeds the cap of %d", max_n, AHC_MAX_POINTS);
    XV_REQUIRE(max_c <= AHC_MAX_N && max_c <= max_n, "ahc_cluster_sums: %d clusters exceed the cap of %d (or the %d rows)", max_c, AHC_MAX_N, max_n);
    XV_REQUIRE(scores && mat_offsets && n && ld && c && members && starts && seed && sizes && status && scores_floats > 0,
               "ahc_cluster_sums: bad arguments");
    XV_REQUIRE(total_n >= b && total_n <= (int64_t)b * max_n && total_c >= b && total_c <= (int64_t)b * max_c && sum_c2 >= total_c &&
               sum_c2 <= total_c * max_c && sum_nc >= total_n && sum_nc <= total_n * max_c,
               "ahc_cluster_sums: total_n / total_c / sum_c2 / sum_nc do not fit b recordings of at most %d rows and %d clusters", max_n, max_c);
    const size_t need = xv_ahc_cluster_sums_workspace_bytes(b, sum_nc);
    XV_REQUIRE(ws && ws_bytes >= need && (uintptr_t)ws % 8 == 0, "ahc_cluster_sums: workspace of %zu bytes, %zu needed (8-byte aligned)", ws_bytes, need);
    AhcSumsArgs g;
    g.scores = scores; g.scores_floats = (long)scores_floats;
    g.mat_offsets = mat_offsets; g.n = n; g.ld = ld; g.c = c; g.members = members; g.starts = starts;
    g.total_n = (long)total_n; g.total_c = (long)total_c; g.sum_c2 = (long)sum_c2; g.sum_nc = (long)sum_nc;
    g.seed = seed; g.sizes = sizes; g.status = status;
    g.rows = (double*)ws; g.plan = (long*)((double*)ws + sum_nc);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ahc_sums_plan_kernel, dim3(b), dim3(AHCS_THREADS), 0, s, g);
    XV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ahc_sums_rows_kernel, dim3(xv_cdiv(max_n, AHCS_ROWS), xv_cdiv(max_c, AHCS_CLUSTERS), b), dim3(AHCS_THREADS), 0, s, g);
    XV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ahc_sums_fold_kernel, dim3(xv_cdiv(max_c, AHCS_THREADS), max_c, b), dim3(AHCS_THREADS), 0, s, g);
    XV_LAUNCH_CHECK();
    return 0;
}

extern "C" int xv_ahc_cut(void* stream, const int32_t* merges, const float* merge_values, const int32_t* n_merges, const int32_t* n, int b,
                          int max_n, int64_t total_n, const float* thresholds, const int32_t* min_clusters, const int32_t* max_clusters, int cuts,
                          int32_t* labels, int32_t* clusters) {
    XV_REQUIRE(b > 0, "ahc_cut: no recording in the call (b=%d)", b);
    XV_REQUIRE(max_n >= 1, "ahc_cut: a recording needs at least one row (largest n=%d)", max_n);
    XV_REQUIRE(max_n <= AHC_MAX_N, "ahc_cut: a recording of %d rows exceeds the cap of %d", max_n, AHC_MAX_N);
    XV_REQUIRE(cuts > 0 && cuts <= 65535, "ahc_cut: 1 .. 65535 cuts in a call (cuts=%d)", cuts);
    XV_REQUIRE(total_n >= b && total_n <= (int64_t)b * max_n, "ahc_cut: total_n does not fit b recordings of at most %d rows", max_n);
    XV_REQUIRE(n_merges && n && thresholds && min_clusters && max_clusters && labels && clusters, "ahc_cut: bad arguments");
    XV_REQUIRE(total_n == b || (merges && merge_values), "ahc_cut: merges and merge_values are needed (some recording has two rows or more)");
    AhcCutArgs g;
    g.merges = merges; g.merge_values = merge_values; g.n_merges = n_merges; g.n = n;
    g.thresholds = thresholds; g.min_clusters = min_clusters; g.max_clusters = max_clusters;
    g.b = b; g.total_n = (long)total_n;
    g.labels = labels; g.clusters = clusters;
    hipLaunchKernelGGL(ahc_cut_kernel, dim3(b, cuts), dim3(AHC_THREADS), 0, (hipStream_t)stream, g);
    XV_LAUNCH_CHECK();
    return 0;
}
