// Photometric confidence of a plane-sweep depth (mv3d/utils.py:111-145, get_propability_map): the probability mass of the two
// depth planes that bracket a pixel's depth.
//
//   soft_argmin_kernel              the regulariser's last kernel: softmax(-x) expectation over the depth planes.
//   soft_argmin_prob_kernel<true>   the same soft-argmin (one walk function, soft_argmin_walk: the depth has the bits
//                                   soft_argmin_kernel writes) that keeps the running maximum m and the denominator den at its
//                                   end, takes the two bracketing planes of its OWN depth, re-reads their two logits and writes
//                                   their softmax values' sum beside the depth.
//   soft_argmin_prob_kernel<false>  the walk for m and den alone (no numerator) and the same tail on a depth map the caller
//                                   gives: the confidence of any depth under the distribution of x_reg.
//   prob_gather_kernel              the reference's function verbatim on a volume that already holds probabilities.
//
// One thread per pixel, lanes along the pixel index: the walk and the stores are coalesced; the two re-reads of a pixel hit the
// column it has just streamed.  No LDS, no atomics, no workspace, no scratch (build-time ISA guard); nothing depends on
// scheduling, so repeated launches are bit-identical.
//
// Arithmetic of the tail (include/v3d.h states it; all fp32, every operation rounded on its own): d = fl(fl(depth -
// depth_start) / depth_interval); l = clamp(floor(d), 0, D - 1), r = clamp(ceil(d), 0, D - 1), clamped as floats before the
// integer conversion; a d that is NaN or infinite gives l = r = 0 and is never converted.
#include <cmath>
#include <cstdint>

#include "costreg.h"

namespace {

constexpr int kTile = 256;    // pixels (= threads) per workgroup

// the two planes that bracket `depth` on the grid depth_start + i * depth_interval, i in [0, D)
__device__ __forceinline__ void bracket(float depth, float depth_start, float depth_interval, int D, int& l, int& r) {
#pragma clang fp contract(off)
  const float d = (depth - depth_start) / depth_interval;
  const float top = (float)(D - 1);                    // exact: D < 2^24 (host check)
  const bool finite = fabsf(d) < INFINITY;             // false for NaN and for +-inf
  l = finite ? (int)fminf(fmaxf(floorf(d), 0.f), top) : 0;
  r = finite ? (int)fminf(fmaxf(ceilf(d), 0.f), top) : 0;
}

// The soft-argmin's walk over the D planes of a pixel's column (mvsnet.py:219-227: p = softmax(-x), depth = sum_d vals[d] p[d])
// in one pass with a running maximum: m = max_d -x_d, den = sum_d e^{-x_d - m} and, with NUM, num = sum_d vals[d] e^{-x_d - m}.
// Every soft-argmin kernel of the library walks with this function: the depth is num / den, with and without the confidence.
template <bool NUM>
__device__ __forceinline__ void soft_argmin_walk(const float* __restrict__ col, const float* __restrict__ vals, int D, int HW, float& m,
                                                 float& num, float& den) {
  m = -INFINITY; num = 0.f; den = 0.f;
  auto step = [&](float xin, float val) __attribute__((always_inline)) {
    const float x = -xin;
    if (x > m) {
      const float sc = expf(m - x);          // exp(-inf) = 0 on the first plane
      if (NUM) num *= sc;
      den *= sc; m = x;
    }
    const float ex = expf(x - m);
    if (NUM) num += val * ex;
    den += ex;
  };
  // 8 planes are requested before the first is consumed (the running-maximum chain is sequential, the loads are not)
  int d = 0;
  for (; d + 8 <= D; d += 8) {
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = __builtin_nontemporal_load(col + (size_t)(d + i) * HW);
#pragma unroll
    for (int i = 0; i < 8; ++i) step(x[i], NUM ? vals[d + i] : 0.f);
  }
  for (; d < D; ++d) step(col[(size_t)d * HW], NUM ? vals[d] : 0.f);
}

// the soft-argmin alone: x_reg [n, D, HW] -> depth [n, HW]
__global__ __launch_bounds__(kTile) void soft_argmin_kernel(const float* __restrict__ reg, const float* __restrict__ vals,
                                                            float* __restrict__ depth, int n, int D, int HW) {
  const size_t gid = (size_t)blockIdx.x * kTile + threadIdx.x;
  if (gid >= (size_t)n * HW) return;
  const int b = gid / HW, pix = gid % HW;
  float m, num, den;
  soft_argmin_walk<true>(reg + (size_t)b * D * HW + pix, vals, D, HW, m, num, den);
  const float e = num / den;
  depth[gid] = e;
}

// OWN: depth = the expectation, written to `depth_out` (vals = the plane depths); else depth = depth_in[pixel]
template <bool OWN>
__global__ __launch_bounds__(kTile) void soft_argmin_prob_kernel(const float* __restrict__ reg, const float* __restrict__ vals,
                                                                 const float* __restrict__ depth_in, float* __restrict__ depth_out,
                                                                 float* __restrict__ prob, float depth_start, float depth_interval,
                                                                 int n, int D, int HW) {
  const size_t gid = (size_t)blockIdx.x * kTile + threadIdx.x;
  if (gid >= (size_t)n * HW) return;
  const int b = gid / HW, pix = gid % HW;
  const float* col = reg + (size_t)b * D * HW + pix;
  float m, num, den;
  soft_argmin_walk<OWN>(col, vals, D, HW, m, num, den);
  float e;
  if (OWN) {
    e = num / den;
    depth_out[gid] = e;
  } else {
    e = depth_in[gid];
  }
  // the two bracketing planes: softmax (divide), gather, add -- the reference's order
  int l, r;
  bracket(e, depth_start, depth_interval, D, l, r);
  const float xl = col[(size_t)l * HW], xr = col[(size_t)r * HW];
  const float pl = expf(-xl - m) / den;
  const float pr = expf(-xr - m) / den;
  prob[gid] = pl + pr;
}

__global__ __launch_bounds__(kTile) void prob_gather_kernel(const float* __restrict__ cv, const float* __restrict__ depth,
                                                            float* __restrict__ prob, float depth_start, float depth_interval, int n,
                                                            int D, int HW) {
  const size_t gid = (size_t)blockIdx.x * kTile + threadIdx.x;
  if (gid >= (size_t)n * HW) return;
  const int b = gid / HW, pix = gid % HW;
  const float* col = cv + (size_t)b * D * HW + pix;
  int l, r;
  bracket(depth[gid], depth_start, depth_interval, D, l, r);
  prob[gid] = col[(size_t)l * HW] + col[(size_t)r * HW];
}

// what the three entry points share: shapes, the plane grid as fp32, the launch size
int check_grid(const char* who, double depth_start, double depth_interval, int n, int D, int H, int W, float* ds, float* di,
               unsigned* blocks) {
  V3D_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0, V3D_ERR_BAD_SHAPE, "%s: n, D, h, w must be positive (got %d, %d, %d, %d)", who, n, D,
              H, W);
  V3D_REQUIRE(D < (1 << 24) && (long long)H * W < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: D = %d / h * w = %lld too large", who, D,
              (long long)H * W);
  const long long nb = ((long long)n * H * W + kTile - 1) / kTile;
  V3D_REQUIRE(nb < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: %lld pixels are too many for one launch", who, (long long)n * H * W);
  *ds = (float)depth_start;
  *di = (float)depth_interval;
  V3D_REQUIRE(std::isfinite(*ds), V3D_ERR_BAD_ARG, "%s: depth_start = %g is not a finite fp32 number", who, depth_start);
  V3D_REQUIRE(std::isfinite(*di) && *di != 0.f, V3D_ERR_BAD_ARG, "%s: depth_interval = %g is zero or not finite as fp32", who,
              depth_interval);
  *blocks = (unsigned)nb;
  return V3D_OK;
}

}  // namespace

namespace v3d {

int launch_soft_argmin(const float* xreg, const float* depth_vals, float* depth, int n, int D, int H, int W, hipStream_t s) {
  const size_t npix = (size_t)n * H * W;
  {
    v3d::TimedScope ts("soft_argmin", s);
    soft_argmin_kernel<<<(unsigned)((npix + 255) / 256), 256, 0, s>>>(xreg, depth_vals, depth, n, D, H * W);
  }
  V3D_CHECK_LAUNCH("soft_argmin_kernel");
  return V3D_OK;
}

int launch_soft_argmin_prob(const float* xreg, const float* depth_vals, float* depth, float* prob, double depth_start,
                            double depth_interval, int n, int D, int H, int W, hipStream_t s) {
  float ds, di;
  unsigned blocks;
  const int rc = check_grid("soft_argmin_prob", depth_start, depth_interval, n, D, H, W, &ds, &di, &blocks);
  if (rc != V3D_OK) return rc;
  {
    v3d::TimedScope ts("soft_argmin_prob", s);
    soft_argmin_prob_kernel<true><<<blocks, kTile, 0, s>>>(xreg, depth_vals, nullptr, depth, prob, ds, di, n, D, H * W);
  }
  V3D_CHECK_LAUNCH("soft_argmin_prob_kernel");
  return V3D_OK;
}

}  // namespace v3d

extern "C" int v3d_confidence_logits_f32(const float* x_reg, const float* depth_map, double depth_start, double depth_interval, int n,
                                         int D, int h, int w, float* prob, void* stream) {
  const char* who = "v3d_confidence_logits_f32";
  V3D_REQUIRE(x_reg && depth_map && prob, V3D_ERR_BAD_ARG, "%s: null argument", who);
  float ds, di;
  unsigned blocks;
  const int rc = check_grid(who, depth_start, depth_interval, n, D, h, w, &ds, &di, &blocks);
  if (rc != V3D_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("confidence_logits", s);
    soft_argmin_prob_kernel<false><<<blocks, kTile, 0, s>>>(x_reg, nullptr, depth_map, nullptr, prob, ds, di, n, D, h * w);
  }
  V3D_CHECK_LAUNCH("soft_argmin_prob_kernel");
  return V3D_OK;
}

extern "C" int v3d_probability_map_f32(const float* cv, const float* depth_map, double depth_start, double depth_interval, int n,
                                       int D, int h, int w, float* prob, void* stream) {
  const char* who = "v3d_probability_map_f32";
  V3D_REQUIRE(cv && depth_map && prob, V3D_ERR_BAD_ARG, "%s: null argument", who);
  float ds, di;
  unsigned blocks;
  const int rc = check_grid(who, depth_start, depth_interval, n, D, h, w, &ds, &di, &blocks);
  if (rc != V3D_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("prob_gather", s);
    prob_gather_kernel<<<blocks, kTile, 0, s>>>(cv, depth_map, prob, ds, di, n, D, h * w);
  }
  V3D_CHECK_LAUNCH("prob_gather_kernel");
  return V3D_OK;
}
