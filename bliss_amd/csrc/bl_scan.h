/*
 * bl_scan.h — what the PCM statistics take from one packed word of two samples: the sums and the central histogram's
 * counts.  Shared by k_pcm_scan (bl_stats_kernels.hip) and k_freq_scan (bl_freq_kernels.hip), where the statistics
 * ride along with the frequency pass, so that both passes are the same arithmetic.  Everything is
 * __device__ __forceinline__; the kernel that includes it owns the LDS the histogram lives in.
 */
#ifndef BL_SCAN_H_
#define BL_SCAN_H_

#include <hip/hip_runtime.h>

#include "bl_device.h"

/* One in-range count of the central histogram for each half of a packed word of two samples: bin = s + 2048 as
 * a 16-bit sum (v_pk_add_u16 for both halves), byte address = base + 4 * bin (v_mad_u32_u16 takes the half it is
 * told to), ds_add_u32.  NO range test: a sample outside [-2048, 2048) gives a bin in [4096, 65536) and an address
 * beyond the workgroup's LDS allocation — the histogram is the LAST thing in it — and the LDS discards
 * out-of-range writes (ISA: DS instructions, out-of-range addresses; checked on the device by
 * tests/test_gpu_parity.py::test_histogram_out_of_range_samples_are_dropped).  4 instructions per word instead of
 * 10 with extraction, compare and exec masks. */
typedef __attribute__((address_space(3))) unsigned bl_lds_u32;
/* What the range-test-free form rests on, checked where it can be: the histogram is the LAST object of the
 * workgroup's LDS (static_asserts at the two kernels that use it; k_pcm_scan also compares its static LDS size at
 * run time), so that 4 * bin >= 4 * BL_HIST_BINS lies behind the allocation or in the allocator's slack, where
 * nothing lives.  -DBL_AMD_CHECKED_HIST (make XDEFS=-DBL_AMD_CHECKED_HIST) builds the kernels with the range compare
 * instead: for debuggers and sanitizers that arm the LDS out-of-range trap. */
__device__ __forceinline__ void scan_hist_word(unsigned w, unsigned lds_base) {
#ifdef BL_AMD_CHECKED_HIST
  const unsigned b0 = (unsigned)((int)(short)(w & 0xFFFFu) + BL_HIST_BINS / 2);
  const unsigned b1 = (unsigned)((int)(short)(w >> 16) + BL_HIST_BINS / 2);
  bl_lds_u32 *h = (bl_lds_u32 *)(size_t)lds_base;
  if (b0 < BL_HIST_BINS) __hip_atomic_fetch_add(h + b0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (b1 < BL_HIST_BINS) __hip_atomic_fetch_add(h + b1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  us2 v;
  __builtin_memcpy(&v, &w, 4);
  v += (us2){BL_HIST_BINS / 2, BL_HIST_BINS / 2};
  unsigned b2;
  __builtin_memcpy(&b2, &v, 4);
  unsigned a0, a1;
  const unsigned one = 1u;
  /* one statement: between two of them hipcc pads with s_nop for hazards it cannot rule out; in this order every
   * address has an instruction between its computation and its use */
  asm volatile("v_mad_u32_u16 %0, %2, 4, %3 op_sel:[0,0,0,0]\n\t"
               "v_mad_u32_u16 %1, %2, 4, %3 op_sel:[1,0,0,0]\n\t"
               "ds_add_u32 %0, %4\n\t"
               "ds_add_u32 %1, %4"
               : "=&v"(a0), "=&v"(a1) : "v"(b2), "v"(lds_base), "v"(one) : "memory");
#endif
}

/* Everything the statistics take from one packed word of two samples: lo + hi into the 32-bit partial sum
 * (v_dot2_i32_i16 with ones), lo^2 + hi^2 (the same instruction; <= 2^31, read as unsigned) into the 64-bit sum of
 * squares by ONE v_mad_u64_u32 (r * 1 + sq; a 64-bit add is two instructions and every one of these issues in four
 * cycles: tools/gen_ubench_issue.py), and the histogram counts: 6 instructions per word. */
__device__ __forceinline__ void scan_word(unsigned w, int &s32, unsigned long long &sq, unsigned lds_hist, bool hist) {
  typedef short short2v __attribute__((ext_vector_type(2)));
  const short2v ones = {1, 1};
  short2v pr;
  __builtin_memcpy(&pr, &w, 4);
  s32 = __builtin_amdgcn_sdot2(pr, ones, s32, false);
  unsigned r; /* the builtin with a zero addend becomes v_mov 0 + v_dot2c: one instruction too many */
  asm("v_dot2_i32_i16 %0, %1, %1, 0" : "=v"(r) : "v"(w));
  asm("v_mad_u64_u32 %0, vcc, %1, 1, %0" : "+v"(sq) : "v"(r) : "vcc");
  if (hist) scan_hist_word(w, lds_hist);
}

#endif /* BL_SCAN_H_ */
