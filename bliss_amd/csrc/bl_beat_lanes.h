/*
 * bl_beat_lanes.h — the cross-lane maximum of the candidate keys that k_beats (bl_beat_kernels.hip) and k_tbeats
 * (bl_tbeats_kernels.hip) share: G = 2^k consecutive lanes own one hop and join their 64-bit keys by DPP inside a row
 * of 16 lanes and by two wave shuffles beyond it.  Device code only.
 */
#ifndef BL_BEAT_LANES_H_
#define BL_BEAT_LANES_H_

#include <hip/hip_runtime.h>

typedef long long bl_i64;
typedef unsigned long long bl_u64;

/* cross-lane move inside a row of 16 lanes: 0xB1 = quad_perm [1,0,3,2], 0x4E = quad_perm [2,3,0,1], 0x141 =
 * row_half_mirror, 0x140 = row_mirror; taken in this order, each once the smaller groups are uniform, every lane of a
 * group of 2, 4, 8 or 16 ends with the group's maximum */
template <int CTRL> __device__ __forceinline__ bl_i64 bt_dpp(bl_i64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(bl_u64)v, CTRL, 0xF, 0xF, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((bl_u64)v >> 32), CTRL, 0xF, 0xF, true);
  return (bl_i64)(((bl_u64)hi << 32) | lo);
}
__device__ __forceinline__ bl_i64 bt_max(bl_i64 a, bl_i64 b) { return a > b ? a : b; }
__device__ __forceinline__ bl_i64 bt_group_max(bl_i64 k, int G) { /* G: uniform over the workgroup */
  if (G >= 2) k = bt_max(k, bt_dpp<0xB1>(k));
  if (G >= 4) k = bt_max(k, bt_dpp<0x4E>(k));
  if (G >= 8) k = bt_max(k, bt_dpp<0x141>(k));
  if (G >= 16) k = bt_max(k, bt_dpp<0x140>(k));
  if (G >= 32) k = bt_max(k, __shfl_xor(k, 16));
  if (G >= 64) k = bt_max(k, __shfl_xor(k, 32));
  return k;
}

#endif /* BL_BEAT_LANES_H_ */
