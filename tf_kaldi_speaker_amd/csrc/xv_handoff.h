// Cross-workgroup hand-over inside one launch and the LDS-DMA address forms (gfx950 only): what the GEMM units, xv_skinny.hip and
// xv_loss.hip share of device-side memory protocol.
#pragma once
#include "xv_common.h"

// ---- cross-workgroup hand-over inside one launch (split sums, last-arriver epilogues)
// Protocol (xv_skinny.hip, xv_loss.hip, xv_gemm_nt.hip): a producer workgroup writes its partial results with xv_handoff_store, every
// storing wave drains them (xv_handoff_drain), the workgroup meets at a barrier, ONE lane takes a ticket (xv_ticket_take); the workgroup
// whose ticket is the last one reads every partial with xv_handoff_load after a second barrier.  All three are RELAXED agent-scope
// atomics: on gfx950 that is `global_store/load ... sc1` (written through to / read from the memory level all XCDs share) and a
// device-scope RMW - exactly the hand-off MI355X_MICROARCH.md ("Valid forms", first row of the sc1 table) measures as valid, and the
// only one that does not pay `buffer_wbl2 sc1` (a write-back of the XCD's WHOLE L2, 12 us per split on the segment kernels) per
// workgroup, which is what a release fence / release RMW lowers to.  Under the HIP memory model alone a relaxed ticket carries no
// happens-before edge, so this is an ARCHITECTURE contract, not a language one: the guard below stops any other target from
// compiling it silently, and tests/test_gpu_ops.py::test_split_handoff_stress replays the hand-over thousands of times
// against the unsplit result.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "xv_handoff_* relies on gfx950 sc1 write-through stores / L2-bypassing loads; re-derive the hand-over for this target"
#endif
__device__ __forceinline__ void xv_handoff_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float xv_handoff_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void xv_handoff_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// 16-byte forms for tile-sized partials (64 KB per workgroup): `global_store_dwordx4 ... sc1` / `global_load_dwordx4 ... sc1` (the widths
// the guide's hand-off table rates fastest: a 4-byte sc1 store costs ~6x the time per byte).  HIP has no 16-byte atomic, so these are
// inline assembly: the compiler does not count them in its own s_waitcnt bookkeeping, which only ever makes ITS waits longer (vmcnt
// retires in issue order); the loads wait for themselves, the stores are drained by xv_handoff_drain.
// The s_nop behind the store is the ISA's "VMEM store of more than 64 bits, then a write of its data VGPRs" hazard (2 wait states):
// hipcc pads it for its own stores but cannot see through inline assembly, and the very next instruction here usually builds the
// next float4 in the same registers.  [measured, round 3: without it one register in sixteen of every shared tile arrived corrupted]
__device__ __forceinline__ void xv_handoff_store4(float* p, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
// eight loads in flight: p + i * stride floats, i = 0..7 (a slab in [register][thread] order: every wave instruction moves 1 KB of
// consecutive bytes - [measured, round 3] with a lane's four float4 side by side, i.e. 16-byte pieces at a 64-byte stride per
// instruction, a shared tile end of the evenly scheduled GEMM cost ~19 us: every piece is a fabric transaction of its own)
__device__ __forceinline__ void xv_handoff_load8(const float* p, int stride, f32x4 (&v)[8]) {
    const float *p1 = p + stride, *p2 = p + 2 * stride, *p3 = p + 3 * stride, *p4 = p + 4 * stride, *p5 = p + 5 * stride, *p6 = p + 6 * stride,
                *p7 = p + 7 * stride;
    asm volatile(
        "global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %9, off sc1\n\t"
        "global_load_dwordx4 %2, %10, off sc1\n\tglobal_load_dwordx4 %3, %11, off sc1\n\t"
        "global_load_dwordx4 %4, %12, off sc1\n\tglobal_load_dwordx4 %5, %13, off sc1\n\t"
        "global_load_dwordx4 %6, %14, off sc1\n\tglobal_load_dwordx4 %7, %15, off sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
        : "v"(p), "v"(p1), "v"(p2), "v"(p3), "v"(p4), "v"(p5), "v"(p6), "v"(p7)
        : "memory");
}

// LDS-DMA of 16 bytes per lane (global_load_lds_dwordx4) in the address form that costs the issuing wave least: a wave-uniform 64-bit
// base in SGPRs + ONE 32-bit byte offset per lane, M0 = the LDS byte address the wave's 1 KB lands at.  [measured, round 3, tdnn2 forward at
// S1, stamps] with per-lane 64-bit addresses (a v_lshl_add_u64 + a two-VGPR address read per instruction, which is what hipcc makes of the
// builtin inside a loop - it folds a scalar base back into the vector address) the MFMA pipe was 0.867 occupied; the same loads fed from one
// hot KiB 0.883 (so it is not the memory side); this form 0.939: 488 -> 449 us, 132 -> 143 TF.  The compiler does not see the loads:
// callers wait with xv_dma_wait_all() before the barrier that publishes a stage, and every operand row must lie within 4 GB of the base.
// (M0 is a reserved register: naming it in the clobber list is rejected.  hipcc sets it immediately in front of each of its own uses and
// keeps nothing in it across statements; the kernels that use this form issue ALL their LDS-DMA through it or xv_dma16_ptr.)
__device__ __forceinline__ void xv_dma16(const float* sbase, unsigned voff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(lds_byte_addr), "v"(voff), "s"(sbase) : "memory");
}
// the same instruction with a 64-bit address per lane (the ragged K-steps, whose out-of-range pieces read a zero page that may lie more
// than 4 GB from the operand).  Every LDS-DMA of these kernels goes through one of the two forms, so hipcc never materialises M0 for a
// DMA of its own in them and cannot hoist or merge an M0 initialisation across these statements.  `lds` = a wave-uniform
// shared-memory pointer.
__device__ __forceinline__ void xv_dma16_ptr(const void* gaddr, const void* lds) {
    const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) const void*)lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(la), "v"(gaddr) : "memory");
}
__device__ __forceinline__ void xv_dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the LDS byte address of a wave-uniform shared-memory pointer, as a scalar
__device__ __forceinline__ unsigned xv_lds_addr(const void* p) {
    return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) const void*)p);
}
// one lane per workgroup, after xv_handoff_drain + __syncthreads(): true for the workgroup that arrives last of `expected`; that
// lane also re-arms the ticket for the next launch (every other arrival has already been counted)
__device__ __forceinline__ bool xv_ticket_take(unsigned* ticket, unsigned expected) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = (t == expected - 1u);
    if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return last;
}
