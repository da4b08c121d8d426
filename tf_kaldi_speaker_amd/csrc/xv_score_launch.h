// The launch side the scoring and back-end units share (xv_score.hip, xv_backend.hip, xv_backend_cohort.hip): operand checks, the choice
// between a row kernel's float4 and scalar form, its launch, the plain NT GEMM into a score slab and the rows of one round of a cohort op.
// Host code only.  gfx950 only.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "xv_common.h"
#include "xv_gemm.h"
#include "xv_rowsum.h"      // SC_ROWS_PER_WG
#include "xv_select.h"      // SC_TILE_ROWS

static inline bool sc_aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }
// [a, a + an) and [b, b + bn) floats share an address
static inline bool sc_overlap(const float* a, size_t an, const float* b, size_t bn) {
    return (uintptr_t)a < (uintptr_t)(b + bn) && (uintptr_t)b < (uintptr_t)(a + an);
}

// a row-wise output y[rows][ldy] of x[rows][ldx], d columns used, and the optional vector v[d] it is computed with: y is x in place with
// the same pitch or shares no address with it, and v lies outside y.  The names are the op's, for its refusals.
static inline int sc_check_row_out(const char* op, const char* xn, const float* x, int ldx, const char* yn, const float* y, int ldy, int rows, int d,
                                   const char* vn, const float* v) {
    XV_REQUIRE((x == y && ldx == ldy) || !sc_overlap(x, (size_t)(rows - 1) * ldx + d, y, (size_t)rows * ldy),
               "%s: %s and %s overlap (in place needs %s == %s and the same pitch)", op, xn, yn, yn, xn);
    XV_REQUIRE(!v || !sc_overlap(v, d, y, (size_t)rows * ldy), "%s: %s and %s overlap", op, vn, yn);
    return 0;
}

// a row kernel takes its float4 form: d and every pitch are multiples of 4 and every pointer (nullptr: not given) is on the 16-byte grid
static inline bool sc_vec_ok(int d, std::initializer_list<long> pitches, std::initializer_list<const void*> ptrs) {
    bool ok = d % 4 == 0;
    for (long p : pitches) ok = ok && p % 4 == 0;
    for (const void* p : ptrs) ok = ok && sc_aligned16(p);
    return ok;
}

template <class T> struct sc_as { using type = T; };      // (the arguments convert to the kernel's parameter types, they do not deduce them)

// One wave per row over `count` rows: the kernel's float4 form kv when vec, else its scalar form ks.  too_many: the op's refusal of a
// count past the grid, a format with one %lld (nullptr where the count is an int, which cannot be).
template <class... A>
static int sc_launch_rows(void (*kv)(A...), void (*ks)(A...), bool vec, long count, const char* too_many, hipStream_t s, typename sc_as<A>::type... args) {
    XV_REQUIRE(count <= (long)SC_ROWS_PER_WG * 0x7fffffff, too_many, (long long)count);
    void (*kernel)(A...) = vec ? kv : ks;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((count + SC_ROWS_PER_WG - 1) / SC_ROWS_PER_WG)), dim3(256), 0, s, args...);
    XV_LAUNCH_CHECK();
    return 0;
}

// C[M][N] = A[M][K] . Bt[N][K]^T, rows lda / ldb / ldc floats apart: xv_affine_forward with k = 1, segs = M, t_in = 1, except that a row
// pitch may exceed K; no scratch: one workgroup per tile
static inline int sc_gemm_nt(hipStream_t s, const float* A, long lda, const float* Bt, long ldb, float* C, long ldc, int M, int N, int K) {
    XvGemmNT g = {};
    g.A = A; g.lda = lda; g.a_rps = 1; g.a_pitch = 1;
    g.Bt = Bt; g.ldb = ldb;
    g.C = C; g.ldc = ldc;
    g.M = M; g.N = N; g.K = K;
    return xv_launch_gemm_nt(s, g);
}

// rows per round of a cohort op: whole GEMM row tiles, as many as the workspace holds (fit) and as the GEMM addresses (its row operand,
// `pitch` floats a row, spans less than 4 GB: xv_launch_gemm_nt; a pitch so long that not even one tile fits under that is refused there)
static inline int sc_tile_rows(size_t fit, size_t pitch) {
    const size_t span = (((size_t)1 << 32) - 1) / (pitch * sizeof(float));
    const size_t cap = span > SC_TILE_ROWS + 1 ? (span - 1) / SC_TILE_ROWS * SC_TILE_ROWS : SC_TILE_ROWS;
    return (int)std::min(std::min(fit / SC_TILE_ROWS * SC_TILE_ROWS, cap), (size_t)1 << 20);
}
