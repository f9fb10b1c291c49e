// Depth supervision of PL3DVNet.forward (mv3d/lightningmodel.py:57-119) in one pass: the masked MAE loss (mv3d/loss.py:6-20) and
// the 2D depth metrics without a mask (mv3d/eval/metricfunctions.py:26-67) of depth maps against ground truth that is reduced to
// the prediction's size by a nearest resize.  include/v3d.h states the rule under v3d_depth_supervision_f32.
//
//   depth_supervision_slice_kernel     one workgroup per slice of kSlice prediction pixels of one image, the image taken as a flat
//                                      h w array.  A lane takes 8 consecutive prediction pixels per step with two 16-byte loads,
//                                      gathers the ground truth through the two resize tables (row_src [h], col_src [w]; none =
//                                      identity) and keeps six double sums and six 32-bit counters: the five and five of the
//                                      metrics (csrc/depth_pixel.h, the rule csrc/depthmetrics.hip uses) and the loss's sum of
//                                      |p - g| and count over g != 0.  Lanes are reduced by wave shuffles, the four waves through
//                                      LDS in wave order; the slice's twelve partials go to the workspace.
//   depth_supervision_finalize_kernel  one workgroup: a thread per image sums that image's slices in slice order and finalises the
//                                      image's row; after a barrier ten threads sum the rows, one column each, in image order.
//
// No atomics and no scratch (build-time ISA guard).  The number of slices depends on h w alone, every order of summation is
// fixed: repeated launches and other devices give the same bits.  Which lane adds which pixel is a function of the pixel's index
// in its image alone, so any alignment of the prediction's base gives the same bits: a slice whose first pixel is not 16-byte
// aligned and the image's last, partial group are read pixel by pixel, by the same lanes in the same order.
//
// The loss has another mask (g != 0, compared in fp32) than the metrics (0.5 <= g < 65): pixels with 0 < g < 0.5 or g >= 65 count
// in the loss and not in the metrics.
#include <cmath>
#include <cstdint>

#include "depth_pixel.h"
#include "v3d_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlice = 8192;      // prediction pixels of one image per workgroup: 10 slices of a 256 x 320 map
constexpr int kGroup = 8;         // consecutive pixels a lane takes per step: two 16-byte loads
constexpr int kSums = 6, kCounts = 6, kCols = 10;

using v3d::depth2d::Acc;
using v3d::depth2d::pixel;

struct Loss {
  double abs;      // sum of |p - g| over g != 0
  int n;           // pixels with g != 0
};

__device__ __forceinline__ void supervise_pixel(Acc& a, Loss& l, float gf, float pf) {
#pragma clang fp contract(off)
  const double g = (double)gf;
  pixel(a, g, pf, 0, (uint8_t)1);
  if (gf != 0.f) {                         // the reference's ~eq(gt, 0): a NaN ground truth is in the mask
    l.abs += fabs((double)pf - g);         // a non-finite term is added as it is
    l.n += 1;
  }
}

__global__ __launch_bounds__(kThreads) void depth_supervision_slice_kernel(const float* __restrict__ pred, int hw, int w,
                                                                           const float* __restrict__ gt, int H, int W,
                                                                           const int32_t* __restrict__ row_src,
                                                                           const int32_t* __restrict__ col_src, int slices,
                                                                           double* __restrict__ part_sums,
                                                                           int32_t* __restrict__ part_counts) {
  struct alignas(16) Vec { float v[4]; };
  const int img = (int)blockIdx.x / slices, sl = (int)blockIdx.x % slices;
  const int e0 = sl * kSlice, e1 = min(e0 + kSlice, hw);
  const float* p = pred + (size_t)img * hw;
  const float* gimg = gt + (size_t)img * H * W;
  // a table entry outside the ground truth (a caller's mistake) is clamped: no read leaves the image
  auto src_row = [&](int r) { return row_src ? min(max(row_src[r], 0), H - 1) : r; };
  auto src_col = [&](int c) { return col_src ? min(max(col_src[c], 0), W - 1) : c; };
  Acc a = {0., 0., 0., 0., 0., 0, 0, 0, 0, 0};
  Loss l = {0., 0};
  // kSlice is a multiple of kGroup and a group is 32 bytes: all whole groups of a slice are 16-byte aligned or none is
  const bool aligned = ((uintptr_t)(p + e0) & 15) == 0;
  const int ngroups = (e1 - e0 + kGroup - 1) / kGroup;
  for (int gi = (int)threadIdx.x; gi < ngroups; gi += kThreads) {
    const int e = e0 + gi * kGroup;
    const int cnt = min(kGroup, e1 - e);
    int r = e / w, c = e - r * w;
    const float* grow = gimg + (size_t)src_row(r) * W;
    if (cnt == kGroup && aligned) {                       // the body: 16-byte loads of the prediction
      Vec pv[2];
      pv[0] = *reinterpret_cast<const Vec*>(p + e);
      pv[1] = *reinterpret_cast<const Vec*>(p + e + 4);
      float gf[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        gf[k] = grow[src_col(c)];
        if (++c == w && k + 1 < kGroup) {                 // a row (or several: w < kGroup) ends inside the group
          c = 0;
          grow = gimg + (size_t)src_row(++r) * W;
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) supervise_pixel(a, l, gf[k], pv[k / 4].v[k % 4]);
    } else {                                              // the image's last, partial group and unaligned slices: pixel by pixel
      for (int k = 0; k < cnt; ++k) {
        supervise_pixel(a, l, grow[src_col(c)], p[e + k]);
        if (++c == w && k + 1 < cnt) {
          c = 0;
          grow = gimg + (size_t)src_row(++r) * W;
        }
      }
    }
  }

  // lanes -> wave (shuffles), waves -> workgroup (LDS, wave order)
  v3d::depth2d::wave_reduce(a);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    l.abs += __shfl_down(l.abs, off);
    l.n += __shfl_down(l.n, off);
  }
  __shared__ double lds_s[kWaves][kSums];
  __shared__ int lds_c[kWaves][kCounts];
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_s[wave][0] = a.rel, lds_s[wave][1] = a.diff, lds_s[wave][2] = a.inv, lds_s[wave][3] = a.sqrel, lds_s[wave][4] = a.sq;
    lds_s[wave][5] = l.abs;
    lds_c[wave][0] = a.pv, lds_c[wave][1] = a.m, lds_c[wave][2] = a.c1, lds_c[wave][3] = a.c2, lds_c[wave][4] = a.c3;
    lds_c[wave][5] = l.n;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = lds_s[0][threadIdx.x];
    int cnt = lds_c[0][threadIdx.x];
    for (int wv = 1; wv < kWaves; ++wv) {
      s += lds_s[wv][threadIdx.x];
      cnt += lds_c[wv][threadIdx.x];
    }
    part_sums[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
    part_counts[(size_t)blockIdx.x * kCounts + threadIdx.x] = cnt;
  }
}

__global__ __launch_bounds__(kThreads) void depth_supervision_finalize_kernel(const double* __restrict__ part_sums,
                                                                              const int32_t* __restrict__ part_counts, int n,
                                                                              int slices, int hw, double depth_interval,
                                                                              int32_t* __restrict__ counts,
                                                                              double* __restrict__ per_image,
                                                                              double* __restrict__ mean) {
#pragma clang fp contract(off)
  for (int img = (int)threadIdx.x; img < n; img += kThreads) {
    double s[kSums] = {0., 0., 0., 0., 0., 0.};
    int c[kCounts] = {0, 0, 0, 0, 0, 0};
    for (int sl = 0; sl < slices; ++sl) {
      const size_t at = (size_t)img * slices + sl;
#pragma unroll
      for (int k = 0; k < kSums; ++k) {
        s[k] += part_sums[at * kSums + k];
        c[k] += part_counts[at * kCounts + k];
      }
    }
#pragma unroll
    for (int k = 0; k < kCounts; ++k) counts[(size_t)img * kCounts + k] = c[k];
    double* row = per_image + (size_t)img * kCols;
    v3d::depth2d::finish_row(s, c, hw, row);
    // the loss's term of this image: the reference's denominator is a float32 tensor, + 1e-7 one fp32 addition; an image
    // without ground truth gives 0 / 1e-7f = 0
    row[9] = (s[5] / depth_interval) / (double)((float)c[5] + 1e-7f);
  }
  __syncthreads();                       // the rows were written by this workgroup: visible to it behind the barrier
  if (threadIdx.x < kCols) {
    double s = 0.;
    for (int img = 0; img < n; ++img) s += per_image[(size_t)img * kCols + threadIdx.x];
    mean[threadIdx.x] = s / (double)n;
  }
}

int slices_of(long long hw) { return (int)((hw + kSlice - 1) / kSlice); }

size_t counts_offset(long long blocks) { return v3d::align_up((size_t)blocks * kSums * sizeof(double), 256); }

}  // namespace

extern "C" size_t v3d_depth_supervision_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0 || (long long)h * w >= (1ll << 24)) return 0;
  const long long blocks = (long long)n * slices_of((long long)h * w);
  return counts_offset(blocks) + v3d::align_up((size_t)blocks * kCounts * sizeof(int32_t), 256);
}

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
  double* part_sums = (double*)workspace;
  int32_t* part_counts = (int32_t*)((char*)workspace + counts_offset(blocks));
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("depth_supervision_slices", s);
    depth_supervision_slice_kernel<<<(unsigned)blocks, kThreads, 0, s>>>(pred, h * w, w, gt, H, W, row_src, col_src, slices,
                                                                         part_sums, part_counts);
  }
  V3D_CHECK_LAUNCH("depth_supervision_slice_kernel");
  {
    v3d::TimedScope ts("depth_supervision_finalize", s);
    depth_supervision_finalize_kernel<<<1, kThreads, 0, s>>>(part_sums, part_counts, n, slices, h * w, (double)depth_interval,
                                                             counts, per_image, mean);
  }
  V3D_CHECK_LAUNCH("depth_supervision_finalize_kernel");
  return V3D_OK;
}
