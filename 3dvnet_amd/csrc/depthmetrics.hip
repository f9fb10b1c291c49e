// 2D depth metrics of predicted depth maps against sensor depth (mv3d/eval/metricfunctions.py:26-67, calc_2d_depth_metrics, as
// mv3d/eval/processresults.py:153-169 reaches it: nearest-enlarged predictions, valid = pred != 0 & ~isinf(pred)) in one pass.
//
//   depth_metrics_slice_kernel<GT>  one workgroup per slice of kSlice ground-truth pixels of one image, the image taken as a flat
//                                   H W array.  A lane takes 8 consecutive pixels per step with 16-byte loads (one for u16,
//                                   two for fp32, four for fp64), gathers the predictions through the two resize tables
//                                   (row_src [H], col_src [W]; none = identity) and keeps five double sums and five 32-bit
//                                   counters.  Lanes are reduced by wave shuffles, the four waves through LDS in wave order; the
//                                   slice's ten partials go to the workspace.
//   depth_metrics_finalize_kernel   one workgroup: a thread per image sums that image's slices in slice order and finalises the
//                                   image's row; after a barrier nine threads sum the rows, one column each, in image order.
//
// No atomics and no scratch (build-time ISA guard).  The number of slices depends on H W alone, every order of summation is
// fixed: repeated launches and other devices give the same bits.
//
// Which lane adds which pixel, and in which order, is a function of the pixel's index in its image alone: group j of 8 pixels
// of a slice belongs to lane j mod 256, the image's last group may be partial.  So the three ground-truth types and any
// alignment of the base give the same bits for the same values (u16 and fp64(u16 / 1000) in particular).  A 16-byte load needs
// a 16-byte-aligned address; groups are 16, 32 or 64 bytes apart, so the whole groups of a slice are aligned together or not
// at all.  A slice that is not (the base pointer only has to be aligned to its own element: gt[1:] of odd-sized u16 images is
// 2-byte aligned) and the partial last group are read pixel by pixel, by the same lanes in the same order.
//
// Arithmetic per pixel (include/v3d.h states it; csrc/depth_pixel.h holds it, shared with csrc/supervision.hip): float64, every
// operation rounded on its own (no contraction of e e + S into an FMA), divisions and the square root are the IEEE ones; the one
// fp32 operation is 1 / p, because the reference's prediction is a float32 tensor there.
#include <cmath>
#include <cstdint>

#include "depth_pixel.h"
#include "v3d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlice = 8192;      // ground-truth pixels of one image per workgroup: 38 slices of a 480 x 640 image
constexpr int kGroup = 8;         // consecutive pixels a lane takes per step, whatever their type: 16 bytes of u16, 32 of fp32, 64 of fp64

using v3d::depth2d::Acc;          // the per-pixel rule, shared with csrc/supervision.hip
using v3d::depth2d::pixel;

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
  constexpr int V = 16 / (int)sizeof(GT);      // elements of one 16-byte load
  struct alignas(16) Vec { GT v[V]; };
  const int img = (int)blockIdx.x / slices, sl = (int)blockIdx.x % slices;
  const int e0 = sl * kSlice, e1 = min(e0 + kSlice, HW);
  const GT* g = gt + (size_t)img * HW;
  const uint8_t* vm = valid_mode == 1 ? valid + (size_t)img * HW : nullptr;
  const float* pimg = pred + (size_t)img * hp * wp;
  // a table entry outside the prediction (a caller's mistake) is clamped: no read leaves the image
  auto src_row = [&](int r) { return row_src ? min(max(row_src[r], 0), hp - 1) : r; };
  auto src_col = [&](int c) { return col_src ? min(max(col_src[c], 0), wp - 1) : c; };
  Acc a = {0., 0., 0., 0., 0., 0, 0, 0, 0, 0};
  // kGroup is a multiple of every V and kSlice of kGroup: all whole groups of a slice are 16-byte aligned or none is
  const bool aligned = ((uintptr_t)(g + e0) & 15) == 0;
  const int ngroups = (e1 - e0 + kGroup - 1) / kGroup;
  for (int gi = (int)threadIdx.x; gi < ngroups; gi += kThreads) {
    const int e = e0 + gi * kGroup;
    const int cnt = min(kGroup, e1 - e);
    int r = e / W, c = e - r * W;
    const float* prow = pimg + (size_t)src_row(r) * wp;
    if (cnt == kGroup && aligned) {                       // the body: 16-byte loads
      Vec gv[kGroup / V];
#pragma unroll
      for (int k = 0; k < kGroup / V; ++k) gv[k] = *reinterpret_cast<const Vec*>(g + e + k * V);
      float pf[kGroup];
      uint8_t vb[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        pf[k] = prow[src_col(c)];
        vb[k] = vm ? vm[e + k] : (uint8_t)1;
        if (++c == W && k + 1 < kGroup) {                 // a row (or several: W < kGroup) ends inside the group
          c = 0;
          prow = pimg + (size_t)src_row(++r) * wp;
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) pixel(a, metres(gv[k / V].v[k % V]), pf[k], valid_mode, vb[k]);
    } else {                                              // the image's last, partial group and unaligned slices: pixel by pixel
      for (int k = 0; k < cnt; ++k) {
        pixel(a, metres(g[e + k]), prow[src_col(c)], valid_mode, vm ? vm[e + k] : (uint8_t)1);
        if (++c == W && k + 1 < cnt) {
          c = 0;
          prow = pimg + (size_t)src_row(++r) * wp;
        }
      }
    }
  }

  // lanes -> wave (shuffles), waves -> workgroup (LDS, wave order)
  v3d::depth2d::wave_reduce(a);
  __shared__ double lds_s[kWaves][5];
  __shared__ int lds_c[kWaves][5];
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_s[wave][0] = a.rel, lds_s[wave][1] = a.diff, lds_s[wave][2] = a.inv, lds_s[wave][3] = a.sqrel, lds_s[wave][4] = a.sq;
    lds_c[wave][0] = a.pv, lds_c[wave][1] = a.m, lds_c[wave][2] = a.c1, lds_c[wave][3] = a.c2, lds_c[wave][4] = a.c3;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    double s = lds_s[0][threadIdx.x];
    int cnt = lds_c[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) {
      s += lds_s[w][threadIdx.x];
      cnt += lds_c[w][threadIdx.x];
    }
    part_sums[(size_t)blockIdx.x * 5 + threadIdx.x] = s;
    part_counts[(size_t)blockIdx.x * 5 + threadIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(kThreads) void depth_metrics_finalize_kernel(const double* __restrict__ part_sums,
                                                                          const int32_t* __restrict__ part_counts, int n, int slices,
                                                                          int HW, int32_t* __restrict__ counts,
                                                                          double* __restrict__ per_image, double* __restrict__ mean) {
#pragma clang fp contract(off)
  for (int img = (int)threadIdx.x; img < n; img += kThreads) {
    double s[5] = {0., 0., 0., 0., 0.};
    int c[5] = {0, 0, 0, 0, 0};
    for (int sl = 0; sl < slices; ++sl) {
      const size_t at = ((size_t)img * slices + sl) * 5;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        s[k] += part_sums[at + k];
        c[k] += part_counts[at + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) counts[(size_t)img * 5 + k] = c[k];
    v3d::depth2d::finish_row(s, c, HW, per_image + (size_t)img * 9);
  }
  __syncthreads();                       // the rows were written by this workgroup: visible to it behind the barrier
  if (threadIdx.x < 9) {
    double s = 0.;
    for (int img = 0; img < n; ++img) s += per_image[(size_t)img * 9 + threadIdx.x];
    mean[threadIdx.x] = s / (double)n;
  }
}

int slices_of(long long HW) { return (int)((HW + kSlice - 1) / kSlice); }

size_t counts_offset(long long blocks) { return v3d::align_up((size_t)blocks * 5 * sizeof(double), 256); }

}  // namespace

extern "C" size_t v3d_depth_metrics_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 24)) return 0;
  const long long blocks = (long long)n * slices_of((long long)H * W);
  return counts_offset(blocks) + v3d::align_up((size_t)blocks * 5 * sizeof(int32_t), 256);
}

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
  double* part_sums = (double*)workspace;
  int32_t* part_counts = (int32_t*)((char*)workspace + counts_offset(blocks));
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("depth_metrics_slices", s);
    if (gt_type == 0)
      depth_metrics_slice_kernel<uint16_t><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const uint16_t*)gt,
                                                                                 pred_valid, valid_mode, H * W, W, slices, part_sums,
                                                                                 part_counts);
    else if (gt_type == 1)
      depth_metrics_slice_kernel<float><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const float*)gt,
                                                                              pred_valid, valid_mode, H * W, W, slices, part_sums,
                                                                              part_counts);
    else
      depth_metrics_slice_kernel<double><<<(unsigned)blocks, kThreads, 0, s>>>(pred, hp, wp, row_src, col_src, (const double*)gt,
                                                                               pred_valid, valid_mode, H * W, W, slices, part_sums,
                                                                               part_counts);
  }
  V3D_CHECK_LAUNCH("depth_metrics_slice_kernel");
  {
    v3d::TimedScope ts("depth_metrics_finalize", s);
    depth_metrics_finalize_kernel<<<1, kThreads, 0, s>>>(part_sums, part_counts, n, slices, H * W, counts, per_image, mean);
  }
  V3D_CHECK_LAUNCH("depth_metrics_finalize_kernel");
  return V3D_OK;
}
