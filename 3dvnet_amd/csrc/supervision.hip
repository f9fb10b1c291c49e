// Depth supervision of PL3DVNet.forward (mv3d/lightningmodel.py:57-119) in one pass: the masked MAE loss (mv3d/loss.py:6-20) and
// the 2D depth metrics without a mask (mv3d/eval/metricfunctions.py:26-67) of depth maps against ground truth that is reduced to
// the prediction's size by a nearest resize.  include/v3d.h states the rule under v3d_depth_supervision_f32.
//
//   depth_supervision_slice_kernel     walks the prediction, gathers the ground truth: the five sums and five counters of the
//                                      metrics, and behind them the loss's sum of |p - g| and count over g != 0
//   depth_supervision_finalize_kernel  ten columns per image (the nine metrics, the loss's term), ten means
//
// The walk, the reduction, the finalize body and the metrics' per-pixel rule are csrc/depth2d.h's, shared with
// csrc/depthmetrics.hip.
//
// The loss has another mask (g != 0, compared in fp32) than the metrics (0.5 <= g < 65): pixels with 0 < g < 0.5 or g >= 65 count
// in the loss and not in the metrics.
#include <cmath>
#include <cstdint>

#include "depth2d.h"
#include "v3d_common.h"

namespace {

using namespace v3d::depth2d;
constexpr int kSums = 6, kCols = 10;
constexpr int kLoss = 5;      // s[kLoss]: sum of |p - g| over g != 0; c[kLoss]: pixels with g != 0; column 9

__device__ __forceinline__ void supervise_pixel(Acc<kSums>& a, float gf, float pf) {
#pragma clang fp contract(off)
  const double g = (double)gf;
  pixel(a, g, pf, 0, (uint8_t)1);
  if (gf != 0.f) {                         // the reference's ~eq(gt, 0): a NaN ground truth is in the mask
    a.s[kLoss] += fabs((double)pf - g);    // a non-finite term is added as it is
    a.c[kLoss] += 1;
  }
}

__global__ __launch_bounds__(kThreads) void depth_supervision_slice_kernel(const float* __restrict__ pred, int hw, int w,
                                                                           const float* __restrict__ gt, int H, int W,
                                                                           const int32_t* __restrict__ row_src,
                                                                           const int32_t* __restrict__ col_src, int slices,
                                                                           double* __restrict__ part_sums,
                                                                           int32_t* __restrict__ part_counts) {
  const int img = (int)blockIdx.x / slices, sl = (int)blockIdx.x % slices;
  Acc<kSums> a = {};
  walk(pred + (size_t)img * hw, hw, w, sl, gt + (size_t)img * H * W, H, W, row_src, col_src, nullptr,
       [&](float p, float g, uint8_t) { supervise_pixel(a, g, p); });
  reduce_store(a, part_sums, part_counts);
}

__global__ __launch_bounds__(kThreads) void depth_supervision_finalize_kernel(const double* __restrict__ part_sums,
                                                                              const int32_t* __restrict__ part_counts, int n,
                                                                              int slices, int hw, double depth_interval,
                                                                              int32_t* __restrict__ counts,
                                                                              double* __restrict__ per_image,
                                                                              double* __restrict__ mean) {
  finalize<kSums, kCols>(part_sums, part_counts, n, slices, hw, counts, per_image, mean, [=](const double* s, const int* c, double* row) {
#pragma clang fp contract(off)
    // the loss's term of this image: the reference's denominator is a float32 tensor, + 1e-7 one fp32 addition; an image
    // without ground truth gives 0 / 1e-7f = 0
    row[9] = (s[kLoss] / depth_interval) / (double)((float)c[kLoss] + 1e-7f);
  });
}

}  // namespace

extern "C" size_t v3d_depth_supervision_workspace_bytes(int n, int h, int w) { return partials_bytes(n, h, w, kSums); }

extern "C" int v3d_depth_supervision_f32(const float* pred, int n, int h, int w, const float* gt, int H, int W,
                                         const int32_t* row_src, const int32_t* col_src, float depth_interval, int32_t* counts,
                                         double* per_image, double* mean, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "v3d_depth_supervision_f32";
  V3D_REQUIRE(pred && gt && counts && per_image && mean && workspace, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE((row_src != nullptr) == (col_src != nullptr), V3D_ERR_BAD_ARG, "%s: row_src and col_src go together", who);
  V3D_REQUIRE(n > 0 && h > 0 && w > 0 && H > 0 && W > 0, V3D_ERR_BAD_SHAPE,
              "%s: n, h, w, H, W must be positive (got %d, %d, %d, %d, %d)", who, n, h, w, H, W);
  V3D_REQUIRE((long long)h * w < (1ll << 24), V3D_ERR_BAD_SHAPE, "%s: h * w = %lld reaches 2^24 (fp32 counts stop being exact)", who,
              (long long)h * w);
  V3D_REQUIRE(row_src || (h == H && w == W), V3D_ERR_BAD_SHAPE, "%s: without tables the ground truth must be %d x %d, got %d x %d",
              who, h, w, H, W);
  V3D_REQUIRE((uintptr_t)pred % 4 == 0 && (uintptr_t)gt % 4 == 0 && (uintptr_t)workspace % 8 == 0, V3D_ERR_BAD_ARG,
              "%s: pred and gt must be aligned to 4 bytes, the workspace to 8", who);
  const int slices = slices_of((long long)h * w);
  const long long blocks = (long long)n * slices;
  V3D_REQUIRE(blocks < (1ll << 31) && (long long)H * W < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: too many pixels for one launch", who);
  V3D_REQUIRE(workspace_bytes >= v3d_depth_supervision_workspace_bytes(n, h, w), V3D_ERR_WORKSPACE_TOO_SMALL,
              "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, v3d_depth_supervision_workspace_bytes(n, h, w));
  const Partials part = carve(workspace, blocks, kSums);
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("depth_supervision_slices", s);
    depth_supervision_slice_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(pred, h * w, w, gt, H, W, row_src, col_src, slices,
                                                                         part.sums, part.counts);
  }
  V3D_CHECK_LAUNCH("depth_supervision_slice_kernel");
  {
    v3d::TimedScope ts("depth_supervision_finalize", s);
    depth_supervision_finalize_kernel<<<1, kThreads, 0, s>>>(part.sums, part.counts, n, slices, h * w, (double)depth_interval,
                                                             counts, per_image, mean);
  }
  V3D_CHECK_LAUNCH("depth_supervision_finalize_kernel");
  return V3D_OK;
}
