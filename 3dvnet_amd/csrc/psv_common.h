// Device functions shared by the plane-sweep kernels (the forward family mapped in psv_variance.hip: warp + variance, sample
// positions) and by the backward walk of variance_backward.h (the gradient of a variance over the edges with respect to the
// features: psv_backward.hip, backproject_backward.hip).  Together with v3d::world_point and v3d::sample_position (v3d_common.h) they are the ONE statement of the sample geometry: the camera blocks, the plane-sweep
// grid, and the bilinear footprint of a sample position.  A kernel that includes this header and calls them sees the
// positions and weights of every other, bit for bit.
#pragma once
#include "v3d_common.h"

namespace v3d {

// Per-image camera block: [0..8] K^-1, [9..17] R, [18..20] t (used when the image is a reference view) and
// [24..35] P = K [R|t] (used when it is a source view).
constexpr int kCamStride = 36;

// The camera block of one image from its K [9], R [9], t [3] (any address space the pointers reach).
__device__ __forceinline__ void cam_block(const float* __restrict__ Kp, const float* __restrict__ Rp,
                                          const float* __restrict__ tp, float* __restrict__ o) {
  // K^-1 in fp64 (adjugate / determinant), rounded to f32 (utils.py:103 torch.inverse)
  double a = Kp[0], bb = Kp[1], c = Kp[2], d = Kp[3], e = Kp[4], f = Kp[5], g = Kp[6], hh = Kp[7], i = Kp[8];
  double det = a * (e * i - f * hh) - bb * (d * i - f * g) + c * (d * hh - e * g);
  double id = 1.0 / det;
  o[0] = (float)((e * i - f * hh) * id);
  o[1] = (float)((c * hh - bb * i) * id);
  o[2] = (float)((bb * f - c * e) * id);
  o[3] = (float)((f * g - d * i) * id);
  o[4] = (float)((a * i - c * g) * id);
  o[5] = (float)((c * d - a * f) * id);
  o[6] = (float)((d * hh - e * g) * id);
  o[7] = (float)((bb * g - a * hh) * id);
  o[8] = (float)((a * e - bb * d) * id);
  for (int k = 0; k < 9; ++k) o[9 + k] = Rp[k];
  for (int k = 0; k < 3; ++k) o[18 + k] = tp[k];
  // projection matrix P = K [R|t] (mvsnet.py:196-197).  torch.bmm evaluates this small batched product with rounded
  // products and sequential additions (no FMA) -- unlike the large K^-1 p / R^T c / P X products, which are FMA chains
  // in k order -- so contraction is switched off here: the sample coordinates then reproduce the reference's bit for bit
  // (scripts/coord_order_probe.py)
  for (int r = 0; r < 3; ++r)
    for (int j = 0; j < 4; ++j) {
      const float b0 = j < 3 ? Rp[0 * 3 + j] : tp[0], b1 = j < 3 ? Rp[1 * 3 + j] : tp[1], b2 = j < 3 ? Rp[2 * 3 + j] : tp[2];
      o[24 + r * 4 + j] = add_rn(add_rn(mul_rn(Kp[r * 3 + 0], b0), mul_rn(Kp[r * 3 + 1], b1)), mul_rn(Kp[r * 3 + 2], b2));
    }
}

// Plane-sweep grid (utils.py:92-94).  Image coordinate of plane-grid column / row g of n over an image axis of N pixels:
// numpy.linspace(0, N-1, n, dtype=float32) -- float64 arithmetic, last sample = stop; step = (N - 1) / (n - 1) in double.
__device__ __forceinline__ float psv_grid_coord(int g, int n, int N, double step) {
  return (n > 1 && g == n - 1) ? (float)(N - 1) : (float)((double)g * step);
}
// Depth of plane d of D: numpy.linspace(z_start, z_end, D, dtype=float32)
__device__ __forceinline__ float psv_plane_depth(int d, int D, double z_start, double z_step, double z_end) {
  return (d == D - 1 && D > 1) ? (float)z_end : (float)(z_start + (double)d * z_step);
}

// Bilinear footprint of one sample (F.grid_sample, align_corners=True, zeros padding; mvsnet.py:209-211).  The sample
// position is clamped to [-1, Wf] x [-1, Hf] first: inside that range nothing changes; outside it every tap of the true
// sample is out of range (result 0), and the clamped sample has weight 1 on out-of-range cells and weight 0 on the others:
// 0 as well.  NaN positions clamp to -1 (fmaxf returns the number).
struct Footprint {
  float x0, y0;                  // nw cell, in [-1, Wf] x [-1, Hf] (integers)
  float w00, w01, w10, w11;      // nw, ne, sw, se weights: the reference's products (x1 - ix)(y1 - iy), ...
};
__device__ __forceinline__ Footprint psv_footprint(float ix, float iy, int Wf, int Hf) {
  ix = fminf(fmaxf(ix, -1.f), (float)Wf);
  iy = fminf(fmaxf(iy, -1.f), (float)Hf);
  Footprint f;
  f.x0 = floorf(ix); f.y0 = floorf(iy);
  const float x1 = f.x0 + 1.f, y1 = f.y0 + 1.f;
  const float wx0 = x1 - ix, wx1 = ix - f.x0, wy0 = y1 - iy, wy1 = iy - f.y0;
  f.w00 = mul_rn(wx0, wy0); f.w01 = mul_rn(wx1, wy0);
  f.w10 = mul_rn(wx0, wy1); f.w11 = mul_rn(wx1, wy1);
  return f;
}

}  // namespace v3d
