// Depth maps of a triangle mesh (mv3d/eval/meshtodepth.py: Renderer / process_scene, there pyrender / OpenGL): vertices and
// triangles in world coordinates + the projections K [R | t] of n views -> depth [n, h, w], the smallest camera-axis depth of
// any fragment at a pixel, 0 where there is none.  The semantics are pinned in include/v3d.h (homogeneous rasterisation, both
// sides, inclusive edges, per-fragment range test as the clip); this file is one way to walk the image under them.
//
//   mesh_render_fill_kernel     depth <- bits of +inf, status <- 0.
//   mesh_render_kernel          one thread per (view, triangle), views on gridDim.y.  A thread fetches its three indices and nine
//                               floats once, then per view projects them (the k-ordered FMA chains of v3d_common.h), forms the
//                               three edge planes A_i and det, and finds the pixels its fragments can lie in: the bounding box of
//                               the three projections widened by one pixel and clamped IN FLOAT to the image -- or the whole
//                               image when a vertex lies before the near plane or a projected value is not finite.  Small boxes
//                               are walked by the thread itself.  Boxes of more than `render_coop` pixels (and every whole-image
//                               one) are handed to the wave: it ballots the lanes that hold one, broadcasts the ten coefficients
//                               and the box from each in turn, and its 64 lanes cover the box as 4 x 16 pixel tiles.
//                               Depths are positive floats, which order as their bit patterns: the pixel is an unsigned 32-bit
//                               atomicMin, so the result does not depend on scheduling, on the threshold or on how many views
//                               share a launch.  A relaxed load in front of the atomic drops fragments that cannot win (the
//                               value at a pixel only ever decreases, so a stale read is only ever too large).
//   mesh_render_resolve_kernel  bits of +inf -> 0.
//
// No workspace, no allocation, no synchronisation, no LDS, no scratch (build-time ISA guard).
#include <climits>
#include <cmath>

#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::dot4h_chain;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kBlock = 256;               // triangles (= threads) per workgroup
constexpr unsigned kInfBits = 0x7f800000u;
constexpr int kStatusBadIndex = V3D_RENDER_STATUS_BAD_INDEX, kStatusNonFinite = V3D_RENDER_STATUS_NON_FINITE;

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

__device__ __forceinline__ bool finite3(float a, float b, float c) {
  return fabsf(a) < INFINITY && fabsf(b) < INFINITY && fabsf(c) < INFINITY;     // a NaN fails
}

// the three edge planes of a projected triangle and its determinant
struct Planes {
  float a0x, a0y, a0z, a1x, a1y, a1z, a2x, a2y, a2z, det;
};
struct Box {
  int x0, x1, y0, y1;       // inclusive; always inside the image
};

// c = a x b, every component fl(fl(p) - fl(q))
__device__ __forceinline__ void cross_rn(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy,
                                         float& cz) {
  cx = sub_rn(mul_rn(ay, bz), mul_rn(az, by));
  cy = sub_rn(mul_rn(az, bx), mul_rn(ax, bz));
  cz = sub_rn(mul_rn(ax, by), mul_rn(ay, bx));
}

__device__ __forceinline__ float plane_rn(float ax, float ay, float az, float px, float py) {
  return add_rn(add_rn(mul_rn(ax, px), mul_rn(ay, py)), az);
}

// the fragment of one triangle at one pixel (include/v3d.h); pix = that pixel's word
__device__ __forceinline__ void shade(const Planes& t, float px, float py, float znear, float zfar, unsigned* pix) {
  const float e0 = plane_rn(t.a0x, t.a0y, t.a0z, px, py);
  const float e1 = plane_rn(t.a1x, t.a1y, t.a1z, px, py);
  const float e2 = plane_rn(t.a2x, t.a2y, t.a2z, px, py);
  const float s = add_rn(add_rn(e0, e1), e2);
  const bool front = e0 >= 0.f && e1 >= 0.f && e2 >= 0.f && s > 0.f;
  const bool back = e0 <= 0.f && e1 <= 0.f && e2 <= 0.f && s < 0.f;
  if (!(front || back)) return;
  const float z = div_rn(t.det, s);
  if (!(z >= znear && z <= zfar)) return;                                      // a NaN fails
  const unsigned zb = __float_as_uint(z);                                     // znear > 0: positive, ordered as its bits
  if (zb < __hip_atomic_load(pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(pix, zb);
}

__global__ __launch_bounds__(kBlock) void mesh_render_fill_kernel(unsigned* __restrict__ depth, int n_pix, int* __restrict__ status) {
  const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (i == 0) *status = 0;
  if (i < n_pix) depth[i] = kInfBits;
}

__global__ __launch_bounds__(kBlock) void mesh_render_resolve_kernel(unsigned* __restrict__ depth, int n_pix) {
  const int i = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  if (i < n_pix && depth[i] == kInfBits) depth[i] = 0u;
}

__global__ __launch_bounds__(kBlock) void mesh_render_kernel(const float* __restrict__ verts, int n_vert,
                                                             const int* __restrict__ tris, int n_tri,
                                                             const float* __restrict__ proj, int n_view, int h, int w, float pc,
                                                             float znear, float zfar, int coop, unsigned* depth, int* status) {
  const int t = (int)blockIdx.x * kBlock + (int)threadIdx.x;
  const int lane = (int)threadIdx.x & 63;
  // the triangle: fetched once, used for every view of this workgroup
  bool have = false;
  float X0 = 0.f, Y0 = 0.f, Z0 = 0.f, X1 = 0.f, Y1 = 0.f, Z1 = 0.f, X2 = 0.f, Y2 = 0.f, Z2 = 0.f;
  if (t < n_tri) {
    const int i0 = tris[3 * (size_t)t], i1 = tris[3 * (size_t)t + 1], i2 = tris[3 * (size_t)t + 2];
    if ((unsigned)i0 >= (unsigned)n_vert || (unsigned)i1 >= (unsigned)n_vert || (unsigned)i2 >= (unsigned)n_vert) {
      atomicOr(status, kStatusBadIndex);
    } else {
      X0 = verts[3 * (size_t)i0], Y0 = verts[3 * (size_t)i0 + 1], Z0 = verts[3 * (size_t)i0 + 2];
      X1 = verts[3 * (size_t)i1], Y1 = verts[3 * (size_t)i1 + 1], Z1 = verts[3 * (size_t)i1 + 2];
      X2 = verts[3 * (size_t)i2], Y2 = verts[3 * (size_t)i2 + 1], Z2 = verts[3 * (size_t)i2 + 2];
      have = finite3(X0, Y0, Z0) && finite3(X1, Y1, Z1) && finite3(X2, Y2, Z2);
      if (!have) atomicOr(status, kStatusNonFinite);
    }
  }
  const float fw1 = (float)(w - 1), fh1 = (float)(h - 1);
  const int hw = h * w;
  for (int view = (int)blockIdx.y; view < n_view; view += (int)gridDim.y) {       // workgroup-uniform: every lane stays in step
    const float* __restrict__ P = proj + (size_t)view * 12;                       // wave-uniform address: scalar loads
    unsigned* img = depth + (size_t)view * hw;
    Planes pl = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Box box = {0, -1, 0, -1};
    bool live = false, whole = false;
    if (have) {
      const float q0x = dot4h_chain(P[0], X0, P[1], Y0, P[2], Z0, P[3]), q0y = dot4h_chain(P[4], X0, P[5], Y0, P[6], Z0, P[7]),
                  q0z = dot4h_chain(P[8], X0, P[9], Y0, P[10], Z0, P[11]);
      const float q1x = dot4h_chain(P[0], X1, P[1], Y1, P[2], Z1, P[3]), q1y = dot4h_chain(P[4], X1, P[5], Y1, P[6], Z1, P[7]),
                  q1z = dot4h_chain(P[8], X1, P[9], Y1, P[10], Z1, P[11]);
      const float q2x = dot4h_chain(P[0], X2, P[1], Y2, P[2], Z2, P[3]), q2y = dot4h_chain(P[4], X2, P[5], Y2, P[6], Z2, P[7]),
                  q2z = dot4h_chain(P[8], X2, P[9], Y2, P[10], Z2, P[11]);
      const bool n0 = q0z < znear, n1 = q1z < znear, n2 = q2z < znear;
      if (!(n0 && n1 && n2)) {                                                    // wholly before the near plane: no fragment
        cross_rn(q1x, q1y, q1z, q2x, q2y, q2z, pl.a0x, pl.a0y, pl.a0z);
        cross_rn(q2x, q2y, q2z, q0x, q0y, q0z, pl.a1x, pl.a1y, pl.a1z);
        cross_rn(q0x, q0y, q0z, q1x, q1y, q1z, pl.a2x, pl.a2y, pl.a2z);
        pl.det = add_rn(add_rn(mul_rn(q0x, pl.a0x), mul_rn(q0y, pl.a0y)), mul_rn(q0z, pl.a0z));
        whole = n0 || n1 || n2 || !(finite3(q0x, q0y, q0z) && finite3(q1x, q1y, q1z) && finite3(q2x, q2y, q2z));
        live = true;
        float bx0 = 0.f, bx1 = fw1, by0 = 0.f, by1 = fh1;
        if (!whole) {
          // every q.z >= znear > 0.  The box stays in float until it is inside the image: a huge quotient is never converted.
          const float u0 = div_rn(q0x, q0z), u1 = div_rn(q1x, q1z), u2 = div_rn(q2x, q2z);
          const float v0 = div_rn(q0y, q0z), v1 = div_rn(q1y, q1z), v2 = div_rn(q2y, q2z);
          bx0 = floorf(fminf(fminf(u0, u1), u2) - pc) - 1.f;
          bx1 = ceilf(fmaxf(fmaxf(u0, u1), u2) - pc) + 1.f;
          by0 = floorf(fminf(fminf(v0, v1), v2) - pc) - 1.f;
          by1 = ceilf(fmaxf(fmaxf(v0, v1), v2) - pc) + 1.f;
          if (bx1 < 0.f || by1 < 0.f || bx0 > fw1 || by0 > fh1) live = false;     // wholly beside the image
          bx0 = fminf(fmaxf(bx0, 0.f), fw1), bx1 = fminf(fmaxf(bx1, 0.f), fw1);   // fmaxf / fminf map a NaN to the bound
          by0 = fminf(fmaxf(by0, 0.f), fh1), by1 = fminf(fmaxf(by1, 0.f), fh1);
        }
        box.x0 = (int)bx0, box.x1 = (int)bx1, box.y0 = (int)by0, box.y1 = (int)by1;
      }
    }
    const bool big = live && (whole || (box.x1 - box.x0 + 1) * (box.y1 - box.y0 + 1) > coop);
    if (live && !big) {
      for (int r = box.y0; r <= box.y1; ++r) {
        const float py = add_rn((float)r, pc);
        for (int c = box.x0; c <= box.x1; ++c) shade(pl, add_rn((float)c, pc), py, znear, zfar, img + r * w + c);
      }
    }
    // the large boxes, one after the other, by the whole wave
    unsigned long long todo = __ballot(big);
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      Planes p;
      p.a0x = __shfl(pl.a0x, src), p.a0y = __shfl(pl.a0y, src), p.a0z = __shfl(pl.a0z, src);
      p.a1x = __shfl(pl.a1x, src), p.a1y = __shfl(pl.a1y, src), p.a1z = __shfl(pl.a1z, src);
      p.a2x = __shfl(pl.a2x, src), p.a2y = __shfl(pl.a2y, src), p.a2z = __shfl(pl.a2z, src);
      p.det = __shfl(pl.det, src);
      const int x0 = __shfl(box.x0, src), x1 = __shfl(box.x1, src), y0 = __shfl(box.y0, src), y1 = __shfl(box.y1, src);
      for (int r = y0 + (lane >> 4); r <= y1; r += 4) {
        const float py = add_rn((float)r, pc);
        for (int c = x0 + (lane & 15); c <= x1; c += 16) shade(p, add_rn((float)c, pc), py, znear, zfar, img + r * w + c);
      }
    }
  }
}

}  // namespace

extern "C" int v3d_mesh_render_depth_f32(const float* verts, int n_vert, const int32_t* tris, int n_tri, const float* projections,
                                         int n_view, int h, int w, double pixel_center, double znear, double zfar, float* depth,
                                         int32_t* status, void* stream) {
  V3D_REQUIRE(verts && tris && projections && depth && status, V3D_ERR_BAD_ARG, "v3d_mesh_render_depth_f32: null argument");
  V3D_REQUIRE(n_vert >= 1 && n_tri >= 1 && n_view >= 1 && h >= 1 && w >= 1, V3D_ERR_BAD_SHAPE,
              "v3d_mesh_render_depth_f32: n_vert=%d n_tri=%d n_view=%d h=%d w=%d (all positive)", n_vert, n_tri, n_view, h, w);
  V3D_REQUIRE((long long)h * w < (1ll << 31) && (long long)n_view * h * w < (1ll << 31), V3D_ERR_BAD_SHAPE,
              "v3d_mesh_render_depth_f32: %d x %d x %d pixels (fewer than 2^31)", n_view, h, w);
  V3D_REQUIRE(n_tri <= INT_MAX - kBlock, V3D_ERR_BAD_SHAPE, "v3d_mesh_render_depth_f32: n_tri=%d", n_tri);
  const float pc = (float)pixel_center, zn = (float)znear, zf = (float)zfar;
  V3D_REQUIRE(std::isfinite(pixel_center) && std::isfinite(znear) && std::isfinite(zfar) && std::isfinite(pc) && std::isfinite(zf),
              V3D_ERR_BAD_ARG, "v3d_mesh_render_depth_f32: pixel_center=%g znear=%g zfar=%g (finite)", pixel_center, znear, zfar);
  V3D_REQUIRE(znear > 0.0 && znear < zfar && zn > 0.f && zn < zf, V3D_ERR_BAD_ARG,
              "v3d_mesh_render_depth_f32: znear=%g zfar=%g (0 < znear < zfar)", znear, zfar);
  hipStream_t s = (hipStream_t)stream;
  const int n_pix = n_view * h * w;
  const int coop = v3d::option(v3d::kOptRenderCoop);
  const unsigned pix_grid = (unsigned)(((long long)n_pix + kBlock - 1) / kBlock);
  const dim3 grid((unsigned)(((long long)n_tri + kBlock - 1) / kBlock), (unsigned)(n_view < 65535 ? n_view : 65535));
  v3d::TimedScope ts("mesh_render", s);
  mesh_render_fill_kernel<<<pix_grid, kBlock, 0, s>>>((unsigned*)depth, n_pix, status);
  V3D_CHECK_LAUNCH("mesh_render_fill_kernel");
  mesh_render_kernel<<<grid, kBlock, 0, s>>>(verts, n_vert, tris, n_tri, projections, n_view, h, w, pc, zn, zf, coop,
                                             (unsigned*)depth, status);
  V3D_CHECK_LAUNCH("mesh_render_kernel");
  mesh_render_resolve_kernel<<<pix_grid, kBlock, 0, s>>>((unsigned*)depth, n_pix);
  V3D_CHECK_LAUNCH("mesh_render_resolve_kernel");
  return V3D_OK;
}
