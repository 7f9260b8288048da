// LDS / buffer-descriptor plumbing shared by the kernels that stage through LDS-DMA and fetch MFMA fragments with the LDS transpose read
// (gfx950).  ONE definition of everything that decides a hazard or a bounds check: the m0 write and its s_nop, the descriptor flags, the
// out-of-range offset, the counted wait in front of a raw barrier.  Per-file build flags (mas_hip/build.py) apply to this code as to
// the rest of the translation unit that includes it.
#pragma once
#include "mas_common.h"
#include <utility>

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

// word 3 of a raw buffer descriptor (DATA_FORMAT = 32 bit, no swizzle, no stride: offsets are plain bytes checked against num_records) --
// the flags argument of __builtin_amdgcn_make_buffer_rsrc and word 3 of rsrc() below
constexpr int BUFFER_RSRC_FLAGS = 0x00020000;
// voffset beyond any descriptor's num_records: a load at it returns zeros (to LDS as well), a store is dropped.  Adding a tile's small
// positive offsets keeps it out of range.
constexpr int OOB_VOFFSET = (int)0x80000000;

// Hand-built descriptor {base, bytes, flags} for the inline-assembly DMA below.  readfirstlane on every word: the "s" constraint needs the
// four words in SGPRs, and a pointer or size that the compiler has routed through a VGPR (a spill, a select) would otherwise be
// legalised with a waterfall loop around EVERY DMA instruction.  The values are wave-uniform by construction.
__device__ __forceinline__ i32x4 rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    i32x4 r = {(int)(unsigned)a, (int)(unsigned)(a >> 32), (int)bytes, BUFFER_RSRC_FLAGS};
    r[0] = __builtin_amdgcn_readfirstlane(r[0]); r[1] = __builtin_amdgcn_readfirstlane(r[1]);
    r[2] = __builtin_amdgcn_readfirstlane(r[2]); r[3] = __builtin_amdgcn_readfirstlane(r[3]);
    return r;
}

// One LDS-DMA piece: 64 lanes x 16 B = 1 KiB.  Contract:
//   * `lds` is a WAVE-UNIFORM LDS byte address (an SGPR: pass it through readfirstlane); lane i's 16 bytes land at lds + 16 i;
//   * `vo` is the PER-LANE byte offset into descriptor `rs`; a lane whose offset is out of range (OOB_VOFFSET) writes ZEROS to its LDS slot;
//   * m0 is clobbered (it carries the LDS address; the s_nop covers the m0-write -> LDS-DMA hazard);
//   * nothing waits: the piece retires in order with the wave's other vector-memory operations, behind a counted s_waitcnt vmcnt(N).
// Inline assembly, not the clang builtin: with the builtin the compiler knows a buffer_load ... lds is pending and puts an
// `s_waitcnt vmcnt(0)` in front of the next transpose read (conv_wgrad_dma.hip has the story).
__device__ __forceinline__ void dma16(i32x4 rs, unsigned lds, int vo) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(lds), "v"(vo), "s"(rs) : "memory", "m0");
}

// LDS transpose read (ds_read_b64_tr_b16; semantics measured in conv_wgrad.hip): 4 x bf16 per lane from the lane's own LDS address
__device__ __forceinline__ s16x4 lds_read_tr16(const unsigned char* a) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a);
}
// an 8 x bf16 MFMA operand from two transpose reads: elements 0-3 from a0, 4-7 from a1
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* a0, const unsigned char* a1) {
    const s16x4 lo = lds_read_tr16(a0);
    const s16x4 hi = lds_read_tr16(a1);
    const __attribute__((ext_vector_type(8))) short v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return *reinterpret_cast<const bf16x8*>(&v);
}

// Counted wait + raw work-group barrier: all but the N youngest vector-memory operations of this wave have retired (in-order VMEM
// retirement), every LDS operation has; then s_barrier WITHOUT the vmcnt(0) that __syncthreads() implies, and a compiler fence.  N is
// an immediate: the kernels select among their own counts with a switch.
#define WAIT_BARRIER(N) do { asm volatile("s_waitcnt vmcnt(" #N ") lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); \
                             asm volatile("" ::: "memory"); } while (0)

// f(std::integral_constant<int, I>{}) for every I of the sequence, in order: a loop whose index is a compile-time constant in the body
template <int... I, typename F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, F&& f) { (f(std::integral_constant<int, I>{}), ...); }
