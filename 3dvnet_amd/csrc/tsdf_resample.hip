// Resampling of TSDF volumes onto another grid (mv3d/eval/tsdf_atlas.py: TSDF.transform :255-338): crop / pad to another
// voxel_dim and origin, and / or a rigid 3 x 4 transform; the first step of the volume metric (eval_tsdf).
//
//   tsdf_resample_kernel     one thread per OUTPUT voxel.  The source coordinate of the voxel is computed once and serves
//                            everything the call resamples: the tsdf (nearest + trilinear + the reference's two rules) and C
//                            fp32 channels (trilinear, zero padding) that share the source grid.
//   volume_resample_nearest_kernel  the same coordinate, one nearest pick per channel, the element copied in its own type
//                            (1, 2, 4 or 8 bytes); optionally a fill value where the voxel lies outside the source volume.
//
// Lanes run along the flat output index, whose fastest axis is z (as in tsdf.hip): writes are coalesced and neighbouring lanes
// read neighbouring source cells.  No coordinate tensor, no LDS, no atomics, no workspace, no scratch (build-time ISA guard);
// nothing depends on scheduling, so repeated launches are bit-identical.
//
// Arithmetic (include/v3d.h states it; all fp32, every operation rounded on its own except the three FMA chains of the
// transform): world = fl(fl(i * voxel_size) + dst_origin); t = M [world; 1] (dot4h_chain); c = fl(fl(t - src_origin) /
// voxel_size); g = fl(fl(fl(2 c) / (D - 1)) - 1); u = grid_sample's un-normalisation of g.  In-bounds tests are taken on the
// floats before any integer conversion: a NaN or an enormous coordinate fails them and is never converted.
#include <cmath>
#include <cstdint>

#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::dot4h_chain;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kTile = 256;    // output voxels (= threads) per workgroup

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// everything a launch needs besides its pointers; by value in the kernel arguments (scalar registers)
struct Grid {
  int n_out, ny, nz;          // output voxels, output y and z sizes
  int sx, sy, sz;             // source sizes
  int align;                  // grid_sample's align_corners
  float voxel_size;
  float dst_origin[3], src_origin[3];
  float m[12];                // 3 x 4, row major
};

struct Coord {
  float u[3];                 // un-normalised source coordinate per axis (x, y, z)
  bool outside;               // some |g_a| >= 1
};

__device__ __forceinline__ float unnormalize(float g, int D, int align) {
  const float g1 = add_rn(g, 1.f);
  if (align) return mul_rn(div_rn(g1, 2.f), (float)(D - 1));
  return div_rn(sub_rn(mul_rn(g1, (float)D), 1.f), 2.f);
}

__device__ __forceinline__ Coord source_coord(const Grid& G, int i) {
  const int xy = i / G.nz, iz = i - xy * G.nz;
  const int ix = xy / G.ny, iy = xy - ix * G.ny;
  const float wx = add_rn(mul_rn((float)ix, G.voxel_size), G.dst_origin[0]);
  const float wy = add_rn(mul_rn((float)iy, G.voxel_size), G.dst_origin[1]);
  const float wz = add_rn(mul_rn((float)iz, G.voxel_size), G.dst_origin[2]);
  const int D[3] = {G.sx, G.sy, G.sz};
  Coord c;
  c.outside = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float t = dot4h_chain(G.m[4 * a], wx, G.m[4 * a + 1], wy, G.m[4 * a + 2], wz, G.m[4 * a + 3]);
    const float v = div_rn(sub_rn(t, G.src_origin[a]), G.voxel_size);
    const float g = sub_rn(div_rn(mul_rn(2.f, v), (float)(D[a] - 1)), 1.f);
    c.outside = c.outside || fabsf(g) >= 1.f;                     // a NaN is not outside (and lies in no bounds below)
    c.u[a] = unnormalize(g, D[a], G.align);
  }
  return c;
}

// flat source index of round-half-even(u), or -1 when it lies outside the volume (decided on the floats)
__device__ __forceinline__ int nearest_index(const Grid& G, const Coord& c) {
  const float rx = __builtin_rintf(c.u[0]), ry = __builtin_rintf(c.u[1]), rz = __builtin_rintf(c.u[2]);
  if (!(rx >= 0.f && ry >= 0.f && rz >= 0.f && rx <= (float)(G.sx - 1) && ry <= (float)(G.sy - 1) && rz <= (float)(G.sz - 1)))
    return -1;
  return ((int)rx * G.sy + (int)ry) * G.sz + (int)rz;
}

// The eight trilinear taps: flat index (-1 outside) and weight.  Tap k = 4 bx + 2 by + bz: the fastest axis z innermost, as
// torch's kernel walks its corners.  Per axis w0 = fl(fl(f + 1) - u), w1 = fl(u - f), f = floor(u); weight =
// fl(fl(wz * wy) * wx).
struct Taps {
  int idx[8];
  float w[8];
};

__device__ __forceinline__ Taps trilinear_taps(const Grid& G, const Coord& c) {
  const int D[3] = {G.sx, G.sy, G.sz};
  float w[3][2];
  int p[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = floorf(c.u[a]), f1 = add_rn(f, 1.f);
    w[a][0] = sub_rn(f1, c.u[a]);
    w[a][1] = sub_rn(c.u[a], f);
    const float last = (float)(D[a] - 1);
    p[a][0] = (f >= 0.f && f <= last) ? (int)f : -1;
    p[a][1] = (f1 >= 0.f && f1 <= last) ? (int)f1 : -1;
  }
  Taps t;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int bx = k >> 2, by = (k >> 1) & 1, bz = k & 1;
    const bool in = p[0][bx] >= 0 && p[1][by] >= 0 && p[2][bz] >= 0;
    t.idx[k] = in ? (p[0][bx] * G.sy + p[1][by]) * G.sz + p[2][bz] : -1;
    t.w[k] = mul_rn(mul_rn(w[2][bz], w[1][by]), w[0][bx]);
  }
  return t;
}

// sum over the taps inside the volume, in tap order, of fl(value * weight), each addition rounded (no contraction): the
// order and the roundings of torch's CPU kernel
__device__ __forceinline__ float trilinear(const float* __restrict__ src, const Taps& t) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (t.idx[k] >= 0) acc = add_rn(acc, mul_rn(src[t.idx[k]], t.w[k]));
  return acc;
}

__global__ __launch_bounds__(kTile) void tsdf_resample_kernel(const float* __restrict__ tsdf_src, const float* __restrict__ attr_src,
                                                               int channels, Grid G, float* __restrict__ tsdf_dst,
                                                               float* __restrict__ attr_dst) {
  // consecutive workgroups of an XCD sit on neighbouring runs of the output: their source cells meet in the same L2
  const int i = v3d::xcd_contiguous_block() * kTile + (int)threadIdx.x;
  if (i >= G.n_out) return;
  const Coord c = source_coord(G, i);
  const Taps t = trilinear_taps(G, c);
  if (tsdf_src) {
    float v = 1.f;                                                // outside the source volume: empty space
    if (!c.outside) {
      const int n = nearest_index(G, c);
      v = n >= 0 ? tsdf_src[n] : 0.f;                             // zero padding
      if (fabsf(v) < 1.f) v = trilinear(tsdf_src, t);             // interpolate near the surface only, never across -1 / +1
    }
    tsdf_dst[i] = v;
  }
  const size_t n_src = (size_t)G.sx * G.sy * G.sz;
  for (int ch = 0; ch < channels; ++ch)
    attr_dst[(size_t)ch * G.n_out + i] = trilinear(attr_src + ch * n_src, t);
}

template <typename T>
__global__ __launch_bounds__(kTile) void volume_resample_nearest_kernel(const T* __restrict__ src, int channels, Grid G,
                                                                         int fill_outside, T fill, T* __restrict__ dst) {
  const int i = v3d::xcd_contiguous_block() * kTile + (int)threadIdx.x;
  if (i >= G.n_out) return;
  const Coord c = source_coord(G, i);
  const int n = nearest_index(G, c);
  const bool filled = fill_outside && c.outside;
  const size_t n_src = (size_t)G.sx * G.sy * G.sz;
  for (int ch = 0; ch < channels; ++ch) {
    T v = filled ? fill : (T)0;                                   // zero padding
    if (!filled && n >= 0) v = src[ch * n_src + n];
    dst[(size_t)ch * G.n_out + i] = v;
  }
}

inline bool finite3(const float* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  if (!a || !b) return false;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

// the checks the two entry points share; fills G
int make_grid(const char* who, int sx, int sy, int sz, double voxel_size, const float* src_origin_host, const float* matrix_host,
              int align_corners, int nx, int ny, int nz, const float* dst_origin_host, Grid* G) {
  V3D_REQUIRE(src_origin_host && matrix_host && dst_origin_host, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(sx >= 2 && sy >= 2 && sz >= 2 && (long long)sx * sy < (1ll << 31) && (long long)sx * sy * sz < (1ll << 31),
              V3D_ERR_BAD_SHAPE, "%s: source volume %d x %d x %d (at least 2 per axis: the coordinates are normalised by size - 1; "
              "fewer than 2^31 voxels)", who, sx, sy, sz);
  V3D_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31),
              V3D_ERR_BAD_SHAPE, "%s: output volume %d x %d x %d (positive, fewer than 2^31 voxels)", who, nx, ny, nz);
  V3D_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0 && std::isfinite((float)voxel_size) && (float)voxel_size > 0.f,
              V3D_ERR_BAD_ARG, "%s: voxel_size=%g (positive and finite)", who, voxel_size);
  V3D_REQUIRE(finite3(src_origin_host, 3) && finite3(dst_origin_host, 3), V3D_ERR_BAD_ARG, "%s: an origin is not finite", who);
  V3D_REQUIRE(finite3(matrix_host, 12), V3D_ERR_BAD_ARG, "%s: the transform is not finite", who);
  G->n_out = nx * ny * nz;
  G->ny = ny;
  G->nz = nz;
  G->sx = sx;
  G->sy = sy;
  G->sz = sz;
  G->align = align_corners ? 1 : 0;
  G->voxel_size = (float)voxel_size;
  for (int k = 0; k < 3; ++k) {
    G->dst_origin[k] = dst_origin_host[k];
    G->src_origin[k] = src_origin_host[k];
  }
  for (int k = 0; k < 12; ++k) G->m[k] = matrix_host[k];
  return V3D_OK;
}

}  // namespace

extern "C" int v3d_tsdf_resample_f32(const float* tsdf_src, const float* attr_src, int channels, int sx, int sy, int sz,
                                     double voxel_size, const float* src_origin_host, const float* matrix_host, int align_corners,
                                     int nx, int ny, int nz, const float* dst_origin_host, float* tsdf_dst, float* attr_dst,
                                     void* stream) {
  const char* who = "v3d_tsdf_resample_f32";
  V3D_REQUIRE((tsdf_src == nullptr) == (tsdf_dst == nullptr), V3D_ERR_BAD_ARG, "%s: tsdf_src and tsdf_dst go together (null argument)",
              who);
  V3D_REQUIRE(channels >= 0, V3D_ERR_BAD_SHAPE, "%s: channels=%d", who, channels);
  V3D_REQUIRE((channels > 0) == (attr_src != nullptr) && (channels > 0) == (attr_dst != nullptr), V3D_ERR_BAD_ARG,
              "%s: attr_src and attr_dst are given exactly when channels > 0 (null argument)", who);
  V3D_REQUIRE(tsdf_src || channels > 0, V3D_ERR_BAD_ARG, "%s: null argument: nothing to resample", who);
  Grid G;
  const int rc = make_grid(who, sx, sy, sz, voxel_size, src_origin_host, matrix_host, align_corners, nx, ny, nz, dst_origin_host, &G);
  if (rc != V3D_OK) return rc;
  const size_t n_src = (size_t)sx * sy * sz, n_dst = (size_t)G.n_out;
  V3D_REQUIRE((long long)channels * (long long)n_src < (1ll << 40) && (long long)channels * (long long)n_dst < (1ll << 40),
              V3D_ERR_BAD_SHAPE, "%s: channels=%d", who, channels);
  const size_t ts = 4 * n_src, td = 4 * n_dst, as = 4 * n_src * channels, ad = 4 * n_dst * channels;
  V3D_REQUIRE(!overlap(tsdf_src, ts, tsdf_dst, td) && !overlap(tsdf_src, ts, attr_dst, ad) && !overlap(attr_src, as, tsdf_dst, td) &&
                  !overlap(attr_src, as, attr_dst, ad) && !overlap(tsdf_dst, td, attr_dst, ad),
              V3D_ERR_BAD_ARG, "%s: source and destination overlap", who);
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(((long long)G.n_out + kTile - 1) / kTile);
  v3d::TimedScope scope("tsdf_resample", s);
  tsdf_resample_kernel<<<grid, kTile, 0, s>>>(tsdf_src, attr_src, channels, G, tsdf_dst, attr_dst);
  V3D_CHECK_LAUNCH("tsdf_resample_kernel");
  return V3D_OK;
}

extern "C" int v3d_volume_resample_nearest(const void* src, int elem_bytes, int channels, int sx, int sy, int sz, double voxel_size,
                                           const float* src_origin_host, const float* matrix_host, int align_corners, int nx, int ny,
                                           int nz, const float* dst_origin_host, int fill_outside, const void* fill_host, void* dst,
                                           void* stream) {
  const char* who = "v3d_volume_resample_nearest";
  V3D_REQUIRE(src && dst, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(elem_bytes == 1 || elem_bytes == 2 || elem_bytes == 4 || elem_bytes == 8, V3D_ERR_BAD_ARG,
              "%s: elem_bytes=%d (1, 2, 4 or 8)", who, elem_bytes);
  V3D_REQUIRE(fill_outside == 0 || fill_outside == 1, V3D_ERR_BAD_ARG, "%s: fill_outside=%d (0 or 1)", who, fill_outside);
  V3D_REQUIRE(!fill_outside || fill_host, V3D_ERR_BAD_ARG, "%s: null argument: fill_outside without fill bytes", who);
  V3D_REQUIRE(channels >= 1, V3D_ERR_BAD_SHAPE, "%s: channels=%d", who, channels);
  Grid G;
  const int rc = make_grid(who, sx, sy, sz, voxel_size, src_origin_host, matrix_host, align_corners, nx, ny, nz, dst_origin_host, &G);
  if (rc != V3D_OK) return rc;
  const size_t n_src = (size_t)sx * sy * sz, n_dst = (size_t)G.n_out;
  V3D_REQUIRE((long long)channels * (long long)n_src < (1ll << 40) && (long long)channels * (long long)n_dst < (1ll << 40),
              V3D_ERR_BAD_SHAPE, "%s: channels=%d", who, channels);
  V3D_REQUIRE(!overlap(src, n_src * channels * elem_bytes, dst, n_dst * channels * elem_bytes), V3D_ERR_BAD_ARG,
              "%s: source and destination overlap", who);
  uint64_t fill = 0;
  if (fill_outside) memcpy(&fill, fill_host, (size_t)elem_bytes);  // little endian: the low bytes are the element
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)(((long long)G.n_out + kTile - 1) / kTile);
  v3d::TimedScope scope("volume_resample_nearest", s);
  switch (elem_bytes) {
    case 1:
      volume_resample_nearest_kernel<uint8_t><<<grid, kTile, 0, s>>>((const uint8_t*)src, channels, G, fill_outside, (uint8_t)fill,
                                                                     (uint8_t*)dst);
      break;
    case 2:
      volume_resample_nearest_kernel<uint16_t><<<grid, kTile, 0, s>>>((const uint16_t*)src, channels, G, fill_outside, (uint16_t)fill,
                                                                      (uint16_t*)dst);
      break;
    case 4:
      volume_resample_nearest_kernel<uint32_t><<<grid, kTile, 0, s>>>((const uint32_t*)src, channels, G, fill_outside, (uint32_t)fill,
                                                                      (uint32_t*)dst);
      break;
    default:
      volume_resample_nearest_kernel<uint64_t><<<grid, kTile, 0, s>>>((const uint64_t*)src, channels, G, fill_outside, fill,
                                                                      (uint64_t*)dst);
  }
  V3D_CHECK_LAUNCH("volume_resample_nearest_kernel");
  return V3D_OK;
}
