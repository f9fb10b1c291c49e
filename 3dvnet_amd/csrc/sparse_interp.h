// The trilinear corner rule of the refinement stage (refinement.py:33-39 feeding MinkowskiInterpolation), stated once for the two
// corner kernels of sparse_interp.hip: interp_corners_kernel (v3d_sparse_interp_f32 and its backward: training) and
// decoder_corner_kernel (v3d_decoder_fused_f32 in decoder.hip: inference).
#pragma once
#include "sparse_hash.h"

namespace v3dinterp {

constexpr float kCornerMax = 60000.f;      // range guard: no corner beyond it is looked up (below zero: v3dhash::kGuard)

struct Level {                  // one hashed level of the sparse U-Net
  v3dhash::HashTable table;
  const float* min_pts;         // [n_batch, 3]
  float res;                    // x.res of the level (= tensor_stride * voxel size)
  float ts, inv_ts;             // tensor stride and its reciprocal (exact when the stride is a power of two)
};
inline Level level_view(const void* table, int n_in, const float* min_pts, float res, int stride) {
  return Level{v3dhash::table_view(const_cast<void*>(table), n_in), min_pts, res, (float)stride, 1.f / (float)stride};
}
inline bool stride_is_pow2(int stride) { return (stride & (stride - 1)) == 0; }      // the host's choice of POW2

struct Corner { int row; float w; };      // feature row (-1: absent, or outside the key range and never looked up) and weight
struct HashFind {       // the probe, unless somebody counts
  __device__ __forceinline__ int operator()(const v3dhash::HashTable& t, unsigned long long key) const { return v3dhash::hash_find(t, key); }
};

// Corner `corner` (bit d set = upper corner on axis d) of the point (px, py, pz) of batch element b: query coordinate
// ((p - min) / x.res) * x.stride in base-voxel units, corner floor(q / ts) ts + {0, ts}^3, weight prod (1 - |q - c| / ts) over x, y, z
// in that order; absent corners contribute nothing (no renormalisation).  POW2: the tensor stride is a power of two (the U-Net's
// 1, 2, 4): x / ts == x * (1 / ts) bit for bit, six of the nine IEEE divisions become multiplications.  `find` is the probe.
template <bool POW2, class Find = HashFind>
__device__ __forceinline__ Corner interp_corner(const Level& L, int b, float px, float py, float pz, int corner, Find find = Find()) {
  const float ts = L.ts, res = L.res, its = L.inv_ts;
  const float* mn = L.min_pts + b * 3;
  const float qx = ((px - mn[0]) / res) * ts, qy = ((py - mn[1]) / res) * ts, qz = ((pz - mn[2]) / res) * ts;
  auto over_ts = [&](float x) __attribute__((always_inline)) { return POW2 ? x * its : x / ts; };
  const float c0 = floorf(over_ts(qx)) * ts + ((corner & 1) ? ts : 0.f);
  const float c1 = floorf(over_ts(qy)) * ts + ((corner & 2) ? ts : 0.f);
  const float c2 = floorf(over_ts(qz)) * ts + ((corner & 4) ? ts : 0.f);
  float w = 1.f;
  w *= 1.f - over_ts(fabsf(qx - c0));
  w *= 1.f - over_ts(fabsf(qy - c1));
  w *= 1.f - over_ts(fabsf(qz - c2));
  int row = -1;
  if (c0 >= -v3dhash::kGuard && c1 >= -v3dhash::kGuard && c2 >= -v3dhash::kGuard && c0 <= kCornerMax && c1 <= kCornerMax && c2 <= kCornerMax)
    row = find(L.table, v3dhash::pack_key(b, (int)c0, (int)c1, (int)c2));
  return Corner{row, w};
}

// decoder_corner_kernel (sparse_interp.hip) for v3d_decoder_fused_f32, which has checked the arguments: out [n_pts * n_hyp][3][8]
int launch_decoder_corners(const Level (&levels)[3], bool pow2, const float* pts, const int64_t* pts_batch, int n_pts, int n_hyp,
                           void* out, hipStream_t s);

}  // namespace v3dinterp
