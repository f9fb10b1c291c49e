// 2D depth metrics of predicted depth maps against sensor depth (mv3d/eval/metricfunctions.py:26-67, calc_2d_depth_metrics, as
// mv3d/eval/processresults.py:153-169 reaches it: nearest-enlarged predictions, valid = pred != 0 & ~isinf(pred)) in one pass.
//
//   depth_metrics_slice_kernel<GT>  walks the ground truth (uint16 millimetres, fp32 or fp64 metres), gathers the prediction and
//                                   takes the optional validity byte of each ground-truth pixel: five sums, five counters
//   depth_metrics_finalize_kernel   nine columns per image, nine means
//
// The walk, the reduction, the finalize body and the per-pixel rule are csrc/depth2d.h's, shared with csrc/supervision.hip.
#include <cmath>
#include <cstdint>

#include "depth2d.h"
#include "v3d_common.h"

namespace {

using namespace v3d::depth2d;
constexpr int kSums = 5, kCols = 9;

__device__ __forceinline__ double metres(uint16_t v) { return (double)v / 1000.0; }      // the reference's division
__device__ __forceinline__ double metres(float v) { return (double)v; }
__device__ __forceinline__ double metres(double v) { return v; }

template <typename GT>
__global__ __launch_bounds__(kThreads) void depth_metrics_slice_kernel(const float* __restrict__ pred, int hp, int wp,
                                                                       const int32_t* __restrict__ row_src,
                                                                       const int32_t* __restrict__ col_src,
                                                                       const GT* __restrict__ gt, const uint8_t* __restrict__ valid,
                                                                       int valid_mode, int HW, int W, int slices,
                                                                       double* __restrict__ part_sums, int32_t* __restrict__ part_counts) {
  const int img = (int)blockIdx.x / slices, sl = (int)blockIdx.x % slices;
  Acc<kSums> a = {};
  walk(gt + (size_t)img * HW, HW, W, sl, pred + (size_t)img * hp * wp, hp, wp, row_src, col_src,
       valid_mode == 1 ? valid + (size_t)img * HW : nullptr,
       [&](GT g, float p, uint8_t vbyte) { pixel(a, metres(g), p, valid_mode, vbyte); });
  reduce_store(a, part_sums, part_counts);
}

__global__ __launch_bounds__(kThreads) void depth_metrics_finalize_kernel(const double* __restrict__ part_sums,
                                                                          const int32_t* __restrict__ part_counts, int n, int slices,
                                                                          int HW, int32_t* __restrict__ counts,
                                                                          double* __restrict__ per_image, double* __restrict__ mean) {
  finalize<kSums, kCols>(part_sums, part_counts, n, slices, HW, counts, per_image, mean, [](const double*, const int*, double*) {});
}

}  // namespace

extern "C" size_t v3d_depth_metrics_workspace_bytes(int n, int H, int W) { return partials_bytes(n, H, W, kSums); }

extern "C" int v3d_depth_metrics_2d(const float* pred, int hp, int wp, const int32_t* row_src, const int32_t* col_src,
                                    const void* gt, int gt_type, const uint8_t* pred_valid, int valid_mode, int n, int H, int W,
                                    int32_t* counts, double* per_image, double* mean, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const char* who = "v3d_depth_metrics_2d";
  V3D_REQUIRE(pred && gt && counts && per_image && mean && workspace, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE((row_src != nullptr) == (col_src != nullptr), V3D_ERR_BAD_ARG, "%s: row_src and col_src go together", who);
  V3D_REQUIRE(n > 0 && H > 0 && W > 0 && hp > 0 && wp > 0, V3D_ERR_BAD_SHAPE,
              "%s: n, H, W, hp, wp must be positive (got %d, %d, %d, %d, %d)", who, n, H, W, hp, wp);
  V3D_REQUIRE((long long)H * W < (1ll << 24), V3D_ERR_BAD_SHAPE, "%s: H * W = %lld reaches 2^24 (fp32 counts stop being exact)", who,
              (long long)H * W);
  V3D_REQUIRE(row_src || (hp == H && wp == W), V3D_ERR_BAD_SHAPE, "%s: without tables the prediction must be %d x %d, got %d x %d",
              who, H, W, hp, wp);
  V3D_REQUIRE(gt_type >= 0 && gt_type <= 2, V3D_ERR_BAD_ARG, "%s: gt_type = %d (0 u16 mm, 1 fp32 m, 2 fp64 m)", who, gt_type);
  V3D_REQUIRE(valid_mode >= 0 && valid_mode <= 2, V3D_ERR_BAD_ARG, "%s: valid_mode = %d (0 none, 1 given, 2 derived)", who, valid_mode);
  V3D_REQUIRE(valid_mode != 1 || pred_valid, V3D_ERR_BAD_ARG, "%s: valid_mode 1 needs pred_valid", who);
  const size_t esize = gt_type == 0 ? 2 : gt_type == 1 ? 4 : 8;
  V3D_REQUIRE((uintptr_t)gt % esize == 0 && (uintptr_t)workspace % 8 == 0, V3D_ERR_BAD_ARG,
              "%s: gt must be aligned to its element, the workspace to 8 bytes", who);
  const int slices = slices_of((long long)H * W);
  const long long blocks = (long long)n * slices;
  V3D_REQUIRE(blocks < (1ll << 31) && (long long)hp * wp < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: too many pixels for one launch", who);
  V3D_REQUIRE(workspace_bytes >= v3d_depth_metrics_workspace_bytes(n, H, W), V3D_ERR_WORKSPACE_TOO_SMALL,
              "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, v3d_depth_metrics_workspace_bytes(n, H, W));
  const Partials part = carve(workspace, blocks, kSums);
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("depth_metrics_slices", s);
    if (gt_type == 0)
      depth_metrics_slice_kernel<uint16_t><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const uint16_t*)gt,
                                                                                 pred_valid, valid_mode, H * W, W, slices, part.sums,
                                                                                 part.counts);
    else if (gt_type == 1)
      depth_metrics_slice_kernel<float><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const float*)gt,
                                                                              pred_valid, valid_mode, H * W, W, slices, part.sums,
                                                                              part.counts);
    else
      depth_metrics_slice_kernel<double><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const double*)gt,
                                                                               pred_valid, valid_mode, H * W, W, slices, part.sums,
                                                                               part.counts);
  }
  V3D_CHECK_LAUNCH("depth_metrics_slice_kernel");
  {
    v3d::TimedScope ts("depth_metrics_finalize", s);
    depth_metrics_finalize_kernel<<<1, kThreads, 0, s>>>(part.sums, part.counts, n, slices, H * W, counts, per_image, mean);
  }
  V3D_CHECK_LAUNCH("depth_metrics_finalize_kernel");
  return V3D_OK;
}
