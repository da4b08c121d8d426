// The per-recording PCA in front of dense PLDA scoring (Kaldi's ivector-plda-scoring-dense --target-energy, as recalled from
// ivector-plda-scoring-dense.cc and restated - nothing is compared with a run of Kaldi): for each recording a PCA of its own vectors, the
// leading directions up to the target energy, the PLDA model projected into that subspace and diagonalised again.  One workgroup of 512
// threads per recording, the recordings of a call side by side.  Synchronisation is __syncthreads only - no grid-wide barrier, no wait on
// another workgroup, no atomics - so one recording cannot stall another, and a result depends on the recording's own inputs alone: every
// sum runs in a fixed order and every matrix element is written by one thread from one formula, the same bits every time and in every slot
// of the batch.  gfx950 only.
//
// include/xvector_hip.h states the arithmetic; tests/pca_plda_ref.py restates it with numpy.linalg.  Everything is computed in DOUBLE from
// the fp32 rows (a product of two fp32 values is exact in double); the outputs are rounded to fp32 once.  For a recording of n rows in D
// dimensions, W and B the within- and between-class covariances of the model (double, from the host):
//   (1) m = (1 / n) sum_t x_t, C = (1 / n) sum_t x_t x_t^T - m m^T: a thread owns 4 x 4 tiles of the upper triangle and walks t upwards.
//   (2) C = P diag(s) P^T by the cyclic Jacobi method below; s sorted descending (ties: the lower index first), negative values floored at 0.
//   (3) E = sum s (in sorted order); dim = 1, e = 0; while (e / E <= target) { e += s[dim - 1]; dim++; }  p = min(dim, D) - one row more
//       than the energy needs, as in Kaldi's loop.  n = 1, or E = 0: p = 0 and nothing else is written.
//   (4) Q = the first p rows of P^T; W' = Q W Q^T, B' = Q B Q^T (the upper triangle computed, the lower mirrored), mu' = Q mu.
//   (5) L = chol(W') (left-looking, a thread per row), T1 = L^-1 (forward substitution, a thread per column);
//       T1 B' T1^T = U diag(psi) U^T by the same Jacobi; psi descending, floored at 0; T' = U^T T1.
//   (6) A = sqrt(D) T' Q [p][D], offset = -T' mu', psi, and the one-utterance tables a = psi / (psi + 1), v = 1 + psi / (psi + 1), iv = 1 / v,
//       g = 1 / (psi + 1), k0 = -0.5 sum ln v + 0.5 sum ln(psi + 1) (sums in ascending index): each rounded to fp32 once.
//
// The eigensolver: two-sided cyclic Jacobi in the parallel round-robin order.  With M = the order m rounded up to even, a sweep has M - 1
// steps; step r rotates the M / 2 disjoint pairs (M - 1, r) and ((r + k) mod (M - 1), (r - k) mod (M - 1)), k = 1 .. M / 2 - 1, a pair
// that holds the padding index M - 1 >= m being skipped.  A pair (p, q), p < q, is rotated when |a_pq| > tau = 2^-60 ||A||_F (the norm of
// the matrix handed in): theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c;
// all columns p, q of A and of V are rotated (a thread per row and pair), then all rows of A (a thread per pair and column); a_pq and a_qp
// are set to 0 and a_pp -= t a_pq, a_qq += t a_pq exactly.  CONVERGENCE: the solver stops after the first sweep that rotates no pair, i.e.
// when every off-diagonal element of the upper triangle is at most 2^-60 ||A||_F - a relative off-diagonal size
// sqrt(sum_{i<j} a_ij^2) / ||A||_F <= 2^-60 m / sqrt(2) < 2^-52 at m = 256.  SWEEP CAP: 40 sweeps (seen: 5 - 16, the most where n << D leaves a large null space);
// a recording that reaches the cap is flagged p = -2 and nothing but its flag is written.  A W' that is not positive definite (a
// model whose W is not) is flagged p = -3.
// The eigenvectors of equal or zero eigenvalues (a p above the rank of C: a direction in C's null space) are whatever this fixed order of
// rotations leaves: arbitrary as in Kaldi, but the same bits every time.
//
// Where the matrices live: the pair (A, V) of an eigenproblem of order m <= 90 in LDS (2 x 90 x 90 doubles = 126.6 KB of the CU's 160 KB: the
// largest round order that leaves room for the vectors and the rotation tables), a larger one in the workspace, through the same flat
// pointers.  The second eigenproblem has order p, which the energy rule keeps small; every other matrix (Q, the products, L, T1, T') is in
// the workspace: four buffers of (D rounded up to 2)^2 doubles per recording.  One workgroup per CU (LDS), 8 waves: profiles/pca_plda_registers.txt.
#include "xv_common.h"

#define PCA_MAX_D 256
#define PCA_MAX_N 2048
#define PCA_THREADS 512
#define PCA_LDS_M 90
#define PCA_MAX_SWEEPS 40
#define PCA_TAU 8.6736173798840355e-19      // 2^-60

struct PcaArgs {
    const float* x; long x_floats;
    const int64_t* x_offsets; const int32_t* n; const int32_t* ld;
    int d; double target;
    const double* w; const double* b; const double* mu;
    int32_t* p; float* a; float* offset; float* psi; float* coef; float* g; float* k0;
    double* s; double* psi64; int32_t* sweeps;
    double* ws;
};

struct PcaShared {
    double ev[PCA_MAX_D];                 // eigenvalues as they sit on the diagonal, then sorted
    double vec[PCA_MAX_D];                // the mean of the rows; later mu'
    double red[PCA_THREADS];
    double c[PCA_MAX_D / 2], s[PCA_MAX_D / 2], dp[PCA_MAX_D / 2], dq[PCA_MAX_D / 2];      // the rotations of a step
    int pp[PCA_MAX_D / 2], qq[PCA_MAX_D / 2], rot[PCA_MAX_D / 2];
    int perm[PCA_MAX_D];                  // perm[k] = the index of the k-th largest eigenvalue
    double scalar;
    int flag;
};

static inline size_t pca_ws_doubles(int b, int d) {
    const size_t m = (size_t)((d + 1) & ~1);
    return 4 * m * m * (size_t)b;
}

// out[i][j] = sum_k L[i * li + k * lk] * R[k * rk + j * rj], k ascending, one fma per step; sym: the upper triangle, mirrored
__device__ __forceinline__ void pca_mm(double* out, int ldo, int rows, int cols, int K, const double* L, long li, long lk, const double* R, long rk,
                                       long rj, bool sym) {
    for (int idx = threadIdx.x; idx < rows * cols; idx += PCA_THREADS) {
        const int i = idx / cols, j = idx - i * cols;
        if (sym && i > j) continue;
        const double* l = L + i * li;
        const double* r = R + j * rj;
        double acc = 0.0;
#pragma unroll 4
        for (int k = 0; k < K; ++k) acc = fma(l[k * lk], r[k * rk], acc);
        out[(long)i * ldo + j] = acc;
        if (sym && i < j) out[(long)j * ldo + i] = acc;
    }
}

// A [m][m] (symmetric, pitch m) -> its eigenvalues on the diagonal, V [m][m] = the eigenvectors in columns.  Returns the sweeps run, -1 at
// the cap.  Every thread of the workgroup calls it; A is complete (a barrier behind its last store) on entry, A and V on return.
__device__ int pca_jacobi(double* A, double* V, int m, PcaShared& sh) {
    const int tid = threadIdx.x;
    const int M = (m + 1) & ~1, half = M / 2;
    double part = 0.0;
    for (int i = tid; i < m * m; i += PCA_THREADS) {
        const double v = A[i];
        part = fma(v, v, part);
        V[i] = i / m == i % m ? 1.0 : 0.0;
    }
    sh.red[tid] = part;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < PCA_THREADS; ++i) total += sh.red[i];
        sh.scalar = PCA_TAU * sqrt(total);
    }
    __syncthreads();
    const double tau = sh.scalar;
    for (int sweep = 1; sweep <= PCA_MAX_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < M - 1; ++r) {
            if (tid < half) {
                const int a = tid == 0 ? M - 1 : (r + tid) % (M - 1), b = tid == 0 ? r : (r + (M - 1) - tid) % (M - 1);
                const int p = min(a, b), q = max(a, b);
                int rot = 0;
                if (q < m) {
                    const double apq = A[p * m + q];
                    if (fabs(apq) > tau) {
                        const double app = A[p * m + p], aqq = A[q * m + q];
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                        const double c = 1.0 / sqrt(fma(t, t, 1.0));
                        sh.c[tid] = c;
                        sh.s[tid] = t * c;
                        sh.dp[tid] = app - t * apq;
                        sh.dq[tid] = aqq + t * apq;
                        rot = 1;
                    }
                }
                sh.pp[tid] = p;
                sh.qq[tid] = q;
                sh.rot[tid] = rot;
                rotated |= rot;
            }
            __syncthreads();
            // columns p, q of A (rows 0 .. m) and of V (rows m .. 2 m): a thread per row and pair, the pairs of a row side by side
            for (int idx = tid; idx < 2 * m * half; idx += PCA_THREADS) {
                const int i = idx / half, k = idx - i * half;
                if (!sh.rot[k]) continue;
                double* row = i < m ? A + i * m : V + (i - m) * m;
                const int p = sh.pp[k], q = sh.qq[k];
                const double c = sh.c[k], s = sh.s[k], x = row[p], y = row[q];
                row[p] = c * x - s * y;
                row[q] = s * x + c * y;
            }
            __syncthreads();
            // rows p, q of A: a thread per pair and column; the 2 x 2 block of the pair itself gets its exact values
            for (int idx = tid; idx < half * m; idx += PCA_THREADS) {
                const int k = idx / m, j = idx - k * m;
                if (!sh.rot[k]) continue;
                const int p = sh.pp[k], q = sh.qq[k];
                const double c = sh.c[k], s = sh.s[k], x = A[p * m + j], y = A[q * m + j];
                double nx = c * x - s * y, ny = s * x + c * y;
                if (j == p) { nx = sh.dp[k]; ny = 0.0; }
                if (j == q) { nx = 0.0; ny = sh.dq[k]; }
                A[p * m + j] = nx;
                A[q * m + j] = ny;
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) return sweep;
    }
    return -1;
}

// the diagonal of A, floored at 0, sorted descending into sh.ev with sh.perm (ties: the lower index first)
__device__ void pca_sorted_eigenvalues(const double* A, int m, PcaShared& sh) {
    const int tid = threadIdx.x;
    if (tid < m) sh.red[tid] = fmax(A[tid * m + tid], 0.0);
    __syncthreads();
    if (tid < m) {
        const double v = sh.red[tid];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += sh.red[j] > v || (sh.red[j] == v && j < tid);
        sh.ev[rank] = v;
        sh.perm[rank] = tid;
    }
    __syncthreads();
}

__global__ __launch_bounds__(PCA_THREADS) void pca_plda_kernel(PcaArgs g) {
    XV_EW_PRIORITY();
    __shared__ __attribute__((aligned(16))) double mat[2 * PCA_LDS_M * PCA_LDS_M];
    __shared__ PcaShared sh;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int n = g.n[r], ld = g.ld[r], D = g.d, D4 = (D + 3) & ~3;
    const long x0 = g.x_offsets[r];
    // a recording whose entries would take the kernel outside the buffer of the call is skipped (ops.backend_pca_plda checks them on the host)
    if (n < 1 || n > PCA_MAX_N || ld < D || x0 < 0 || x0 > g.x_floats || x0 + (long)(n - 1) * ld + D > g.x_floats) {
        if (tid == 0) g.p[r] = -1;
        return;
    }
    const float* __restrict__ X = g.x + x0;
    const long mm = (long)((D + 1) & ~1) * ((D + 1) & ~1);
    double* R0 = g.ws + 4 * mm * r;
    double* R1 = R0 + mm;
    double* R2 = R1 + mm;
    double* R3 = R2 + mm;
    double* s_out = g.s + (long)r * D;

    // (1) the mean and the covariance
    if (tid < D) {
        double acc = 0.0;
        for (int t = 0; t < n; ++t) acc += (double)X[(long)t * ld + tid];
        sh.vec[tid] = acc / (double)n;
    }
    __syncthreads();
    double* A = D <= PCA_LDS_M ? mat : R0;
    double* V = D <= PCA_LDS_M ? mat + D * D : R1;
    {
        const int nt = (D + 3) / 4;
        for (int idx = tid; idx < nt * nt; idx += PCA_THREADS) {
            const int ti = idx / nt, tj = idx - ti * nt;
            if (ti > tj) continue;
            const int i0 = 4 * ti, j0 = 4 * tj;
            double acc[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
            for (int t = 0; t < n; ++t) {
                const float* xr = X + (long)t * ld;
                double a[4], b[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a[u] = i0 + u < D ? (double)xr[i0 + u] : 0.0;
                    b[u] = j0 + u < D ? (double)xr[j0 + u] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int i = i0 + u, j = j0 + v;
                    if (i < D && j < D && i <= j) {
                        const double c = acc[u][v] / (double)n - sh.vec[i] * sh.vec[j];
                        A[i * D + j] = c;
                        A[j * D + i] = c;
                    }
                }
        }
    }
    __syncthreads();

    // (2) C = P diag(s) P^T
    const int sweeps1 = pca_jacobi(A, V, D, sh);
    if (sweeps1 < 0) {
        if (tid == 0) g.p[r] = -2;
        return;
    }
    pca_sorted_eigenvalues(A, D, sh);
    if (tid < D) s_out[tid] = sh.ev[tid];

    // (3) the kept dimension
    if (tid == 0) {
        double total = 0.0;
        for (int k = 0; k < D; ++k) total += sh.ev[k];
        int dim = 0;
        if (n > 1 && total > 0.0) {
            double e = 0.0;
            dim = 1;
            while (dim <= D && e / total <= g.target) {
                e += sh.ev[dim - 1];
                ++dim;
            }
            dim = min(dim, D);
        }
        sh.flag = dim;
    }
    __syncthreads();
    const int p = sh.flag;
    if (p == 0) {
        if (tid == 0) { g.p[r] = 0; g.sweeps[2 * r] = sweeps1; g.sweeps[2 * r + 1] = 0; }
        return;
    }

    // (4) Q [p][D] = the leading eigenvectors in rows; mu', W', B'
    double* Q = R2;
    for (int idx = tid; idx < p * D; idx += PCA_THREADS) {
        const int k = idx / D, j = idx - k * D;
        Q[idx] = V[j * D + sh.perm[k]];
    }
    __syncthreads();      // (everybody has read sh.perm and the mean)
    if (tid < p) {
        double acc = 0.0;
        for (int j = 0; j < D; ++j) acc = fma(Q[tid * D + j], g.mu[j], acc);
        sh.vec[tid] = acc;
    }
    pca_mm(R3, D, p, D, D, Q, D, 1, g.w, D, 1, false);      // Y = Q W
    __syncthreads();
    pca_mm(R0, p, p, p, D, R3, D, 1, Q, 1, D, true);        // W' = Y Q^T
    __syncthreads();
    pca_mm(R3, D, p, D, D, Q, D, 1, g.b, D, 1, false);      // Y = Q B
    __syncthreads();
    pca_mm(R1, p, p, p, D, R3, D, 1, Q, 1, D, true);        // B' = Y Q^T
    __syncthreads();

    // (5) L = chol(W') in place (lower), T1 = L^-1
    double* Lm = R0;
    if (tid == 0) sh.flag = 0;
    for (int j = 0; j < p; ++j) {
        double v = 0.0;
        if (tid >= j && tid < p) {
            v = Lm[tid * p + j];
            for (int k = 0; k < j; ++k) v = fma(-Lm[tid * p + k], Lm[j * p + k], v);
            if (tid == j) {
                if (!(v > 0.0)) sh.flag = 1;
                sh.scalar = sqrt(v);
            }
        }
        __syncthreads();
        if (tid >= j && tid < p) Lm[tid * p + j] = tid == j ? sh.scalar : v / sh.scalar;
        __syncthreads();
    }
    if (sh.flag) {      // (uniform: read behind a barrier)
        if (tid == 0) g.p[r] = -3;
        return;
    }
    double* T1 = R3;
    if (tid < p) {      // column tid of L^-1
        const int c = tid;
        for (int i = 0; i < c; ++i) T1[i * p + c] = 0.0;
        T1[c * p + c] = 1.0 / Lm[c * p + c];
        for (int i = c + 1; i < p; ++i) {
            double acc = 0.0;
            for (int k = c; k < i; ++k) acc = fma(Lm[i * p + k], T1[k * p + c], acc);
            T1[i * p + c] = -acc / Lm[i * p + i];
        }
    }
    __syncthreads();
    double* tmp = R0;      // (L is dead behind the barrier above)
    pca_mm(tmp, p, p, p, p, T1, p, 1, R1, p, 1, false);      // T1 B'
    __syncthreads();
    double* A2 = p <= PCA_LDS_M ? mat : R1;                  // (B' is dead)
    double* V2 = p <= PCA_LDS_M ? mat + p * p : R0;          // (T1 B' is dead once G is formed: pca_jacobi writes V behind the barrier)
    pca_mm(A2, p, p, p, p, tmp, p, 1, T1, 1, p, true);       // G = (T1 B') T1^T
    __syncthreads();
    const int sweeps2 = pca_jacobi(A2, V2, p, sh);
    if (sweeps2 < 0) {
        if (tid == 0) g.p[r] = -2;
        return;
    }
    pca_sorted_eigenvalues(A2, p, sh);      // (sh.vec, mu', is left alone)
    double* Us = R1;      // [p][p]: row i = the eigenvector of the i-th largest psi (G, if it was here, is dead: its diagonal is in sh.ev)
    for (int idx = tid; idx < p * p; idx += PCA_THREADS) {
        const int i = idx / p, k = idx - i * p;
        Us[idx] = V2[k * p + sh.perm[i]];
    }
    __syncthreads();
    double* Tp = R0;      // T' = U^T T1 (V2, if it was here, is dead)
    pca_mm(Tp, p, p, p, p, Us, p, 1, T1, p, 1, false);
    __syncthreads();

    // (6) the outputs
    const double root_d = sqrt((double)D);
    float* a_out = g.a + (long)r * D4 * D4;
    for (int idx = tid; idx < D4 * D4; idx += PCA_THREADS) {
        const int i = idx / D4, j = idx - i * D4;
        double acc = 0.0;
        if (i < p && j < D) {
            for (int k = 0; k < p; ++k) acc = fma(Tp[i * p + k], Q[k * D + j], acc);
            acc *= root_d;
        }
        a_out[idx] = (float)acc;
    }
    if (tid < D4) {
        const long o = (long)r * D4 + tid;
        double off = 0.0, psi = 0.0, a = 0.0, iv = 0.0, gg = 0.0;
        if (tid < p) {
            for (int k = 0; k < p; ++k) off = fma(Tp[tid * p + k], sh.vec[k], off);
            off = -off;
            psi = sh.ev[tid];
            const double v = 1.0 + psi / (psi + 1.0);
            a = psi / (psi + 1.0);
            iv = 1.0 / v;
            gg = 1.0 / (psi + 1.0);
            g.psi64[(long)r * D + tid] = psi;
        }
        g.offset[o] = (float)off;
        g.psi[o] = (float)psi;
        g.coef[2 * (long)r * D4 + tid] = (float)a;
        g.coef[(2 * (long)r + 1) * D4 + tid] = (float)iv;
        g.g[o] = (float)gg;
    }
    if (tid == 0) {
        double lv = 0.0, lp = 0.0;
        for (int k = 0; k < p; ++k) {
            const double psi = sh.ev[k];
            lv += log(1.0 + psi / (psi + 1.0));
            lp += log(psi + 1.0);
        }
        g.k0[r] = (float)(-0.5 * lv + 0.5 * lp);
        g.sweeps[2 * r] = sweeps1;
        g.sweeps[2 * r + 1] = sweeps2;
        g.p[r] = p;
    }
}

extern "C" size_t xv_backend_pca_plda_workspace_bytes(int b, int d) {
    if (b <= 0 || d <= 0 || d > PCA_MAX_D) return 0;
    return pca_ws_doubles(b, d) * sizeof(double);
}

extern "C" int xv_backend_pca_plda(void* stream, const float* x, int64_t x_floats, const int64_t* x_offsets, const int32_t* n, const int32_t* ld,
                                   int b, int d, int max_n, double target, const double* w, const double* bt, const double* mu, int32_t* p,
                                   float* a, float* offset, float* psi, float* coef, float* g, float* k0, double* s, double* psi64,
                                   int32_t* sweeps, void* ws, size_t ws_bytes) {
    XV_REQUIRE(b > 0, "backend_pca_plda: no recording in the call (b=%d)", b);
    XV_REQUIRE(d >= 1 && d <= PCA_MAX_D, "backend_pca_plda: d must lie in 1 .. %d (got %d)", PCA_MAX_D, d);
    XV_REQUIRE(max_n >= 1, "backend_pca_plda: a recording needs at least one row (largest n=%d)", max_n);
    XV_REQUIRE(max_n <= PCA_MAX_N, "backend_pca_plda: a recording of %d rows exceeds the cap of %d", max_n, PCA_MAX_N);
    XV_REQUIRE(target > 0.0 && target <= 1.0, "backend_pca_plda: target must lie in (0, 1] (got %g)", target);
    XV_REQUIRE(x && x_offsets && n && ld && w && bt && mu && p && a && offset && psi && coef && g && k0 && s && psi64 && sweeps && x_floats > 0,
               "backend_pca_plda: bad arguments");
    const size_t need = pca_ws_doubles(b, d) * sizeof(double);
    XV_REQUIRE(ws && ws_bytes >= need && ((uintptr_t)ws & 15) == 0, "backend_pca_plda: workspace of %zu bytes, %zu needed, 16-byte aligned", ws_bytes,
               need);
    PcaArgs q;
    q.x = x; q.x_floats = (long)x_floats;
    q.x_offsets = x_offsets; q.n = n; q.ld = ld;
    q.d = d; q.target = target;
    q.w = w; q.b = bt; q.mu = mu;
    q.p = p; q.a = a; q.offset = offset; q.psi = psi; q.coef = coef; q.g = g; q.k0 = k0;
    q.s = s; q.psi64 = psi64; q.sweeps = sweeps;
    q.ws = (double*)ws;
    hipLaunchKernelGGL(pca_plda_kernel, dim3(b), dim3(PCA_THREADS), 0, (hipStream_t)stream, q);
    XV_LAUNCH_CHECK();
    return 0;
}
