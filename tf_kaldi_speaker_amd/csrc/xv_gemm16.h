// Split-precision ("f16x3") MFMA GEMMs: fp32 tensors carried as TWO planes of fp16 pieces so the big
// contractions of the TDNN run on the 16-bit matrix cores (16x the fp32-input MFMA rate) at fp32-class
// accuracy.
//
//   x * s = h + l + eps,   h = fp16(x*s),  l = fp16(x*s - h),   |eps| <= 2^-22 |x*s|
//   a.b  ~=  (ha.hb + ha.lb + la.hb) / (sa*sb)      three fp16 MFMAs per block, fp32 accumulate: v_mfma_f32_16x16x32_f16 in the
//                                                   context-window and weight-gradient kernels, v_mfma_f32_32x32x16_f16 in the generic one
//
// s is a power of two per tensor (exact to apply and undo) chosen from the tensor's max |x| so that
// max |x*s| lies in [2^12, 2^13): 3 bits below the fp16 maximum, and the low piece of every element that
// matters stays a normal fp16.  The max is produced by whoever writes the tensor (exact output range of
// BN+ReLU from the GEMM epilogue's column min/max; a bound for the BN backward; a reduction for inputs and
// weights) and travels as the uint bits of a float in device memory - no host round trip.
// Measured on MI355X (tests/test_gpu_ops_f16x3.py, tools/bench_kernel.py gemm16): max error vs float64 5e-7..8e-7 of the output scale (fp32-input MFMA:
// 1.7e-7), 2.6-3.0x the speed of the fp32-input MFMA kernels of xv_gemm_nt.hip / xv_gemm_tn.hip.
//
// Plane layout: [2][rows][ld] 16-bit, channel axis contiguous, ld a multiple of 8 (16-byte chunks), zero padded.
// The spliced (context-window) row map of xv_gemm_nt.hip applies unchanged to both NT kernels.
//
// Units: xv_planes16.hip (the producers of planes), xv_gemm16_nt.hip (forward and data gradient), xv_gemm16_tn.hip (weight gradient).
// This header holds what more than one of them uses.  The launch structs and launchers are xv_gemm.h's; out-of-range pieces of a ragged
// stage read xv_zero_page() (xv_gemm.h), 16 bytes per lane.
#pragma once
#include "xv_common.h"
#include "xv_epilogue.h"       // xv_pow2_scale, the tile epilogues
#include "xv_gemm.h"
#include "xv_gemm_tile.h"      // xcd_swizzle
#include "xv_handoff.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

// the workgroup barrier of the staging pipelines: xv_dma16's loads are inline assembly the compiler does not count
__device__ __forceinline__ void xv16_sync() {
    xv_dma_wait_all();
    __syncthreads();
}

// One accumulator block's step: af / bf = [plane (0: high, 1: low)][block] 16-byte fragments.  Three MFMAs, cross terms first, then the
// leading product.  (Macros: textual, so every kernel keeps the statements it had.)
#define XV16_MFMA3(MFMA, acc, af, bf, a, b)                                                                    \
    (acc = MFMA(__builtin_bit_cast(f16x8, af[0][a]), __builtin_bit_cast(f16x8, bf[1][b]), acc, 0, 0, 0),       \
     acc = MFMA(__builtin_bit_cast(f16x8, af[1][a]), __builtin_bit_cast(f16x8, bf[0][b]), acc, 0, 0, 0),       \
     acc = MFMA(__builtin_bit_cast(f16x8, af[0][a]), __builtin_bit_cast(f16x8, bf[0][b]), acc, 0, 0, 0))
#define XV16_MFMA3_32X32X16(acc, af, bf, a, b) XV16_MFMA3(__builtin_amdgcn_mfma_f32_32x32x16_f16, acc, af, bf, a, b)      // acc: f32x16
#define XV16_MFMA3_16X16X32(acc, af, bf, a, b) XV16_MFMA3(__builtin_amdgcn_mfma_f32_16x16x32_f16, acc, af, bf, a, b)      // acc: f32x4
