/*
 * bl_desc_pair.h — the pair arithmetic of two descriptors, shared by bl_desc_kernels.hip (k_desc_knn) and
 * bl_desc_chain_kernels.hip (k_desc_chain, k_desc_chain_step): the byte planes of a 16-byte slice, the norm of a
 * vector from its int16, and the constants of a 16 x 16 tile and of a key.  The comment at the head of
 * bl_desc_kernels.hip says what the planes are and how the three int8 matrix products pair them.  Device code only.
 */
#ifndef BL_DESC_PAIR_H_
#define BL_DESC_PAIR_H_

#include <hip/hip_runtime.h>

typedef unsigned long long ds_u64;
typedef int ds_v4i __attribute__((ext_vector_type(4)));

#define DS_TILE 16      /* candidates per step: the columns of a tile */
#define DS_IDX_BITS 27  /* index bits of a key */
#define DS_IDX_MASK ((1u << DS_IDX_BITS) - 1u)

/* 8 int16 (4 words as loaded) -> the planes of h and of l, byte e of word i = dimension 4 i + e of the 8.  The +128 of
 * h = (q + 128) >> 8 is added per half word without a carry between the halves. */
__device__ __forceinline__ void ds_planes(const uint4 w, int (&h)[2], int (&l)[2]) {
  const unsigned v[4] = {w.x, w.y, w.z, w.w};
  unsigned t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = ((v[i] & 0x7FFF7FFFu) + 0x00800080u) ^ (v[i] & 0x80008000u);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    l[i] = (int)__builtin_amdgcn_perm(v[2 * i + 1], v[2 * i], 0x06040200u);
    h[i] = (int)__builtin_amdgcn_perm(t[2 * i + 1], t[2 * i], 0x07050301u);
  }
}

/* sum of the squares of the wave's four slices of a vector, in every lane of the vector's four: a word's two squares
 * are at most 2 * 32512^2 < 2^31 and two words' fit 32 bits unsigned (|q| <= 32768 would still fit 64 below) */
__device__ __forceinline__ ds_u64 ds_norm(const uint4 w) {
  const unsigned v[4] = {w.x, w.y, w.z, w.w};
  ds_u64 s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int a = (int)(short)(v[i] & 0xFFFFu), b = (int)v[i] >> 16;
    s += (ds_u64)(unsigned)(a * a) + (ds_u64)(unsigned)(b * b);
  }
  s += (ds_u64)__shfl_xor(s, 16);
  s += (ds_u64)__shfl_xor(s, 32);
  return s;
}

__device__ __forceinline__ long ds_pack(const int (&p)[2]) {
  return (long)(((ds_u64)(unsigned)p[1] << 32) | (unsigned)p[0]);
}

#endif /* BL_DESC_PAIR_H_ */
