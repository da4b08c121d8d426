// The order-preserving unsigned key of a float, for exact rank selection by radix histogram (xv_score.hip: the top-k cohort scores;
// xv_cm_encode.hip: the quartiles of a 'CM ' column header).  a < b as floats <=> sc_key(a) < sc_key(b) as unsigned, for every pair of
// non-NaN values but the two zeros (-0 sorts below +0); sc_unkey gives the float back bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// the unsigned key whose order is the float's: negative values have every bit flipped, the others the sign bit set
__device__ __forceinline__ unsigned sc_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sc_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
