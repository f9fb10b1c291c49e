// TSDF integration of depth maps (mv3d/eval/tsdf_atlas.py: TSDFFusion.integrate :390-443, get_tsdf :453-463): the depth maps of
// a scene -> a truncated signed distance volume with weights and, optionally, summed colours.
//
//   tsdf_integrate_kernel  one thread per voxel walks the views in order and keeps its five running values (tsdf sum, weight,
//                          three colour sums) in registers; the volume is read once and written once, in place.  Lanes run along
//                          the flat voxel index, whose fastest axis is z: the volume traffic is coalesced and neighbouring lanes
//                          project to neighbouring texels.  The camera rows of a view sit at a wave-uniform address (scalar
//                          loads).  No atomics, no LDS, no scratch (build-time ISA guard); the chain per voxel is sequential, so
//                          one launch of N views gives the bits of N launches of one view, and repeated launches are
//                          bit-identical.
//   tsdf_normalize_kernel  sum / weight where weight > 0, a copy elsewhere.
//
// Arithmetic (all fp32; DESIGN.md §2 for the convention): world coordinate = fl(fl(i * voxel_size) + origin) per axis, two
// roundings as the reference's separate multiply and add give; camera rows as k-ordered FMA chains whose homogeneous term is a
// rounded addition; IEEE divisions for u, v and the truncated distance; round-half-even for the texel.  The in-view test is
// taken on the float values, before any integer conversion: a NaN or an enormous coordinate fails it and is never converted.
//
// Culling: a view is skipped for a whole wave before the two divisions when no lane has c2 > 0, and the gather runs only in
// lanes that passed the in-view test.  Both use the per-voxel fp32 verdict itself, so they cannot change a result.
#include <cmath>

#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::dot4h_chain;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kTile = 256;    // voxels (= threads) per workgroup

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

template <bool COLOR>
__global__ __launch_bounds__(kTile) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight,
                                                                float* __restrict__ color, int n_vox, int ny, int nz, float voxel_size,
                                                                float ox, float oy, float oz, float trunc_margin,
                                                                const float* __restrict__ proj, const float* __restrict__ depths,
                                                                const float* __restrict__ images, int n, int h, int w) {
  // consecutive workgroups of an XCD sit on neighbouring runs of the volume: their texels meet in the same L2
  const int i = v3d::xcd_contiguous_block() * kTile + (int)threadIdx.x;
  if (i >= n_vox) return;
  const int xy = i / nz, iz = i - xy * nz;
  const int ix = xy / ny, iy = xy - ix * ny;
  const float wx = add_rn(mul_rn((float)ix, voxel_size), ox);
  const float wy = add_rn(mul_rn((float)iy, voxel_size), oy);
  const float wz = add_rn(mul_rn((float)iz, voxel_size), oz);

  float t = tsdf[i], wt = weight[i];
  float cr = 0.f, cg = 0.f, cb = 0.f;
  if (COLOR) {
    cr = color[i];
    cg = color[(size_t)n_vox + i];
    cb = color[2 * (size_t)n_vox + i];
  }
  const float fw = (float)w, fh = (float)h;
  const size_t hw = (size_t)h * w;
  for (int k = 0; k < n; ++k) {
    const float* __restrict__ P = proj + (size_t)k * 12;          // wave-uniform address: scalar loads
    const float c2 = dot4h_chain(P[8], wx, P[9], wy, P[10], wz, P[11]);
    if (!__any(c2 > 0.f)) continue;                               // the whole wave lies behind this camera
    const float c0 = dot4h_chain(P[0], wx, P[1], wy, P[2], wz, P[3]);
    const float c1 = dot4h_chain(P[4], wx, P[5], wy, P[6], wz, P[7]);
    const float px = __builtin_rintf(div_rn(c0, c2)), py = __builtin_rintf(div_rn(c1, c2));
    // a NaN coordinate fails every comparison
    if (!(px >= 0.f && py >= 0.f && px < fw && py < fh && c2 > 0.f)) continue;
    const size_t texel = (size_t)k * hw + (size_t)((int)py * w + (int)px);
    const float d = depths[texel];
    if (!(d > 0.f)) continue;
    const float q = div_rn(sub_rn(d, c2), trunc_margin);
    const float dist = q > 1.f ? 1.f : q;                         // clamp(max = 1); a NaN stays a NaN and fails the next test
    if (!(dist > -1.f)) continue;
    t = wt == 0.f ? dist : add_rn(t, dist);
    wt = add_rn(wt, 1.f);
    if (COLOR) {
      const float* __restrict__ img = images + (size_t)k * 3 * hw + (texel - (size_t)k * hw);
      cr = add_rn(cr, img[0]);
      cg = add_rn(cg, img[hw]);
      cb = add_rn(cb, img[2 * hw]);
    }
  }
  tsdf[i] = t;
  weight[i] = wt;
  if (COLOR) {
    color[i] = cr;
    color[(size_t)n_vox + i] = cg;
    color[2 * (size_t)n_vox + i] = cb;
  }
}

__global__ __launch_bounds__(kTile) void tsdf_normalize_kernel(const float* __restrict__ tsdf_sum, const float* __restrict__ weight,
                                                                const float* __restrict__ color_sum, int n_vox,
                                                                float* __restrict__ tsdf_out, float* __restrict__ color_out) {
  const int i = (int)blockIdx.x * kTile + (int)threadIdx.x;
  if (i >= n_vox) return;
  const float wt = weight[i];
  const bool seen = wt > 0.f;
  const float t = tsdf_sum[i];
  tsdf_out[i] = seen ? div_rn(t, wt) : t;
  if (color_sum) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = color_sum[c * (size_t)n_vox + i];
      color_out[c * (size_t)n_vox + i] = seen ? div_rn(v, wt) : v;
    }
  }
}

inline bool positive_finite(double v) { return std::isfinite(v) && v > 0.0 && std::isfinite((float)v) && (float)v > 0.f; }

}  // namespace

extern "C" int v3d_tsdf_integrate_f32(float* tsdf, float* weight, float* color, int nx, int ny, int nz, double voxel_size,
                                      const float* origin_host, double trunc_margin, const float* projections, const float* depths,
                                      const float* images, int n, int h, int w, void* stream) {
  V3D_REQUIRE(tsdf && weight && origin_host, V3D_ERR_BAD_ARG, "v3d_tsdf_integrate_f32: null argument");
  V3D_REQUIRE((color == nullptr) == (images == nullptr) || n == 0, V3D_ERR_BAD_ARG,
              "v3d_tsdf_integrate_f32: images and the colour volume go together");
  V3D_REQUIRE(positive_finite(voxel_size) && positive_finite(trunc_margin), V3D_ERR_BAD_ARG,
              "v3d_tsdf_integrate_f32: voxel_size=%g trunc_margin=%g (positive and finite)", voxel_size, trunc_margin);
  V3D_REQUIRE(std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]), V3D_ERR_BAD_ARG,
              "v3d_tsdf_integrate_f32: origin is not finite");
  V3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31),
              V3D_ERR_BAD_SHAPE, "v3d_tsdf_integrate_f32: volume %d x %d x %d (positive, fewer than 2^31 voxels)", nx, ny, nz);
  V3D_REQUIRE(n >= 0, V3D_ERR_BAD_SHAPE, "v3d_tsdf_integrate_f32: n=%d", n);
  if (n == 0) return V3D_OK;
  V3D_REQUIRE(projections && depths, V3D_ERR_BAD_ARG, "v3d_tsdf_integrate_f32: null argument");
  V3D_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < (1ll << 31), V3D_ERR_BAD_SHAPE,
              "v3d_tsdf_integrate_f32: h=%d w=%d (positive, fewer than 2^31 pixels)", h, w);
  hipStream_t s = (hipStream_t)stream;
  const int n_vox = nx * ny * nz;
  const unsigned grid = (unsigned)(((long long)n_vox + kTile - 1) / kTile);
  v3d::TimedScope ts("tsdf_integrate", s);
  if (color)
    tsdf_integrate_kernel<true><<<grid, kTile, 0, s>>>(tsdf, weight, color, n_vox, ny, nz, (float)voxel_size, origin_host[0],
                                                       origin_host[1], origin_host[2], (float)trunc_margin, projections, depths,
                                                       images, n, h, w);
  else
    tsdf_integrate_kernel<false><<<grid, kTile, 0, s>>>(tsdf, weight, nullptr, n_vox, ny, nz, (float)voxel_size, origin_host[0],
                                                        origin_host[1], origin_host[2], (float)trunc_margin, projections, depths,
                                                        nullptr, n, h, w);
  V3D_CHECK_LAUNCH("tsdf_integrate_kernel");
  return V3D_OK;
}

extern "C" int v3d_tsdf_normalize_f32(const float* tsdf_sum, const float* weight, const float* color_sum, int n_vox,
                                      float* tsdf_out, float* color_out, void* stream) {
  V3D_REQUIRE(tsdf_sum && weight && tsdf_out, V3D_ERR_BAD_ARG, "v3d_tsdf_normalize_f32: null argument");
  V3D_REQUIRE((color_sum == nullptr) == (color_out == nullptr), V3D_ERR_BAD_ARG,
              "v3d_tsdf_normalize_f32: color_sum and color_out go together");
  V3D_REQUIRE(n_vox >= 1, V3D_ERR_BAD_SHAPE, "v3d_tsdf_normalize_f32: n_vox=%d", n_vox);
  hipStream_t s = (hipStream_t)stream;
  v3d::TimedScope ts("tsdf_normalize", s);
  tsdf_normalize_kernel<<<(unsigned)(((long long)n_vox + kTile - 1) / kTile), kTile, 0, s>>>(tsdf_sum, weight, color_sum, n_vox,
                                                                                            tsdf_out, color_out);
  V3D_CHECK_LAUNCH("tsdf_normalize_kernel");
  return V3D_OK;
}
