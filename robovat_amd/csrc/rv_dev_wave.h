// rv_dev_wave.h -- the lane-phase macros and the cross-lane primitives of the kernels: ONE home, so that whoever writes
// a kernel finds here which primitive exists already.  Device only, except the lane-phase macros (the host emulation
// runs a phase as a loop over 64 lanes).  Helpers that belong to one feature stay with it: pr_argmin
// (rv_dev_push_route.h), the reductions of rv_dev_grasp_sampler.h and rv_dev_plan.h.
// Same value under two names, left as they are for a later change (merging them must keep the generated code):
//   uni(x) and RV_UNI(x);  row_ror_min<N>(x) and fminr(row_ror_f<N>(x), x);  row_ror_add<N>(x) and row_ror_f<N>(x) + x.
#pragma once
#include "rv_dev_math.h"

namespace rv {

#if RV_ON_DEVICE
// The env program runs with ONE wave per workgroup (k_env: __launch_bounds__(RV_ENV_THREADS)), and the LDS operations
// of one wave complete in the order they were issued.  What a lane phase stored is therefore seen by the loads of the
// next phase without waiting for the stores to finish: a phase boundary only has to stop the COMPILER from moving LDS
// accesses across it (a wavefront-scope fence + wave_barrier; no instruction).  __syncthreads() would add the
// workgroup-scope fence, an s_waitcnt lgkmcnt(0) that exposes one LDS store latency per boundary.  It stays where
// global memory is ordered or a workgroup holds several waves (rv_env_kernel.h, the other kernels).
// (FLAT accesses that land in LDS are NOT in that order.  The only ones of the env program are the hull-vertex reads of
// the out-of-line epa(), behind GJK iterations that have read the same arrays with DS loads and used the values.)
#define RV_ENV_THREADS 64
static_assert(RV_ENV_THREADS == 64, "RV_WAVE_SYNC is a phase boundary only while a workgroup of k_env is one wave64");
#define RV_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define RV_LANES_BEGIN { const int lane = (int)threadIdx.x;
#define RV_LANES_END } RV_WAVE_SYNC();
// a value every lane holds alike (read from the env's LDS block), moved to the scalar unit so that the control flow
// that hangs on it is compiled as uniform
#define RV_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
#else
#define RV_UNI(x) ((int)(x))
#define RV_LANES_BEGIN for (int lane = 0; lane < 64; ++lane) {
#define RV_LANES_END }
#endif

#if RV_ON_DEVICE
// ---- one lane to the scalar unit / to every lane ----
RV_DEV int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
RV_DEV float unif(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
RV_DEV float rdlane(float x, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l)); }
RV_DEV v3 rdlane3(v3 x, int l) { return mk(rdlane(x.x, l), rdlane(x.y, l), rdlane(x.z, l)); }
// ---- within a 16-lane group (one DPP row) ----
// "is it this lane's turn" of the lane-per-row sweeps: (lane's row) == s for a compile-time s.  The compare is loop
// invariant, so the compiler computes the 12 (36) lane masks once, keeps them in SGPR pairs -- and, out of SGPRs, spills them
// into a VGPR: every row step then paid two v_readlane + a wait state to get its mask back.  An opaque copy of the lane's
// row index makes the compare part of the step: v_cmp_eq (inline constant) + v_cndmask through vcc, two instructions.
RV_DEV int opaque_i(int x) {
#if RV_ON_DEVICE
  asm volatile("" : "+v"(x));
#endif
  return x;
}
// lane S of the caller's own 16-lane group, to every lane of the group: the DPP control row_newbcast:S (gfx90a and
// later: "broadcast lane S of each row of 16 to the whole row") -- ONE VALU instruction; no trip through SGPRs, and not
// the ~100 clocks of the LDS crossbar that the ds_swizzle of the first version took on the critical path of every row step
template <int S_> RV_DEV float grp_bcast(float x) {
  const int xi = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, 0x150 + S_, 0xf, 0xf, true));
}
template <int N_> RV_DEV int grp_ror_max(int x) {       // max with the lane N_ to the right in the 16-lane row (row_ror)
  const int y = __builtin_amdgcn_update_dpp(x, x, 0x120 + N_, 0xf, 0xf, true);
  return x > y ? x : y;
}
template <int N> RV_DEV float row_ror_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, false));
}
template <int N> RV_DEV int row_ror_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x120 + N, 0xf, 0xf, false); }
// max with the lane N to the right in the 16-lane row: v_max_f32 on the rotated value (equal to the ternary for every
// finite input up to the sign of a zero; support_v of rv_dev_collide.h says why that cannot be seen there)
// (ONE instruction, v_max_f32_dpp, behind the two wait states a DPP read of a just-written VGPR needs.  Through
// __builtin_fmaxf(update_dpp(0, x), x) a step was five issue slots: the move of the `old' operand, the wait state, the DPP
// move, a v_max x, x that quiets a possible signalling NaN of the moved value, and the maximum itself)
template <int N> RV_DEV float row_ror_fmax(float x) {
  float r;
  if (N == 8) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else if (N == 4) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else if (N == 2) asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  else asm("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 row_ror:1 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x));
  return r;
}
template <int N> RV_DEV int row_ror_imin(int x) {
  int o = row_ror_i<N>(x);
  return o < x ? o : x;
}
template <int N> RV_DEV float row_ror_min(float x) {
  float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, false));
  return o < x ? o : x;
}
template <int N> RV_DEV float row_ror_add(float x) {
  float o = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, false));
  return o + x;
}
// ---- where the wave runs ----
// which XCD (0 .. 7), read from the hardware: a fact about where the wave is, not an assumption about dispatch
RV_DEV int rv_xcc_id() {
  unsigned x;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  return (int)(x & 7u);
}
// ---- a launch argument, read where it is used ----
// The value at byte `off` of the kernel's argument segment.  The segment's address passes through an empty asm first, so
// the load stays HERE: an argument that only the end of a long kernel wants is otherwise loaded at its entry and kept --
// in the env kernel that is one more register spilled around the substep loop per argument
template <typename T> RV_DEV T rv_kernarg_at(int off) {
  typedef const char __attribute__((address_space(4))) kbyte;
  kbyte* p = (kbyte*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const T __attribute__((address_space(4)))*)(p + off);
}
// ---- over the whole wave ----
RV_DEV float wave_min(float x) { for (int o = 32; o > 0; o >>= 1) { float y = __shfl_xor(x, o); x = y < x ? y : x; } return x; }
RV_DEV float wave_max(float x) { for (int o = 32; o > 0; o >>= 1) { float y = __shfl_xor(x, o); x = y > x ? y : x; } return x; }
#endif

}  // namespace rv
