// Decoded frames -> the tensors of a scene batch (mv3d/dsets/dataset.py:75-91, :159-219): the crop, the resize and the colour
// normalisation of the colour frames, and the conversion and the two nearest resizes of the depth frames, each as one gather.
//
//   frames_to_images_kernel   uint8 [n, H, W, 3] (interleaved, channel order as stored) -> fp32 [n, 3, oh, ow].  One thread per
//                             four consecutive output columns of one row of one image: the taps of a column are four pixels
//                             (two source rows x two source columns) of three bytes each, read with byte loads; the twelve
//                             results leave as three 16-byte stores, one per channel plane, consecutive across the wave.  Where
//                             the rows of the output are not 16-byte aligned (ow % 4 != 0, or a base that is not) the same
//                             thread stores its columns one by one and the last thread of a row stops at ow.
//   frames_to_depths_kernel   uint16 millimetres [n, H, W] -> fp32 metres [n, oh, ow]: one thread per output element.
//
// The host computes the gather tables in float64 (3dvnet_amd/dataset.py: PreprocessImage.linear_tables / nearest_tables), so
// the kernels hold no coordinate arithmetic; a table entry outside the frame is clamped to it, so no entry makes a kernel read
// outside `frames` / `depth_mm`.  No LDS, no atomics, no workspace, no scratch (build-time ISA guard); nothing depends on
// scheduling, so repeated launches are bit-identical.  Offsets are 64-bit throughout.
//
// Arithmetic of a colour element (include/v3d.h states it): fp32, every operation rounded on its own, no fused multiply-add, IEEE
// divisions.
#include <cmath>
#include <cstdint>

#include "v3d_common.h"

namespace {

constexpr int kTile = 256;    // threads per workgroup
constexpr int kCols = 4;      // output columns per thread of the colour kernel

struct ColourNorm {
  float scale, mean[3], std[3];
};

// a (1 - w) + b w: one subtraction, two products, one addition, each rounded
__device__ __forceinline__ float lerp_rn(float a, float b, float w) {
#pragma clang fp contract(off)
  const float u = 1.0f - w;
  const float p = a * u;
  const float q = b * w;
  return p + q;
}

// the reference's chain (dataset.py:197, :202-205) on a resized grey level
__device__ __forceinline__ float normalise(float v, float scale, float mean, float std) {
#pragma clang fp contract(off)
  float x = v / 255.0f;
  x = x * 255.0f;
  x = x / scale;
  x = x - mean;
  return x / std;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// VEC: every output row starts on a 16-byte boundary and ow % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(kTile) void frames_to_images_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ y0,
                                                                 const int32_t* __restrict__ y1, const float* __restrict__ wy,
                                                                 const int32_t* __restrict__ x0, const int32_t* __restrict__ x1,
                                                                 const float* __restrict__ wx, float* __restrict__ images,
                                                                 ColourNorm nrm, int quantize, unsigned long long n_threads, int H,
                                                                 int W, int oh, int ow, int groups) {
  const unsigned long long gid = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
  if (gid >= n_threads) return;
  const unsigned long long rowid = gid / (unsigned)groups;         // img * oh + r
  const int c0 = (int)(gid - rowid * (unsigned)groups) * kCols;
  const unsigned long long img = rowid / (unsigned)oh;
  const int r = (int)(rowid - img * (unsigned)oh);
  const uint8_t* frame = frames + (size_t)img * H * W * 3;
  const uint8_t* top = frame + (size_t)clampi(y0[r], H - 1) * W * 3;
  const uint8_t* bot = frame + (size_t)clampi(y1[r], H - 1) * W * 3;
  const float fy = wy[r];
  float v[3][kCols];
#pragma unroll
  for (int j = 0; j < kCols; ++j) {
    const int c = VEC ? c0 + j : min(c0 + j, ow - 1);              // a ragged last thread repeats the last column and drops it below
    const int xa = clampi(x0[c], W - 1) * 3, xb = clampi(x1[c], W - 1) * 3;
    const float fx = wx[c];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float t = lerp_rn((float)top[xa + ch], (float)top[xb + ch], fx);
      const float b = lerp_rn((float)bot[xa + ch], (float)bot[xb + ch], fx);
      float g = lerp_rn(t, b, fy);
      if (quantize) g = rintf(g);
      v[ch][j] = normalise(g, nrm.scale, nrm.mean[ch], nrm.std[ch]);
    }
  }
  const size_t plane = (size_t)oh * ow;
  float* out = images + (size_t)img * 3 * plane + (size_t)r * ow + c0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    if (VEC) {
      *reinterpret_cast<float4*>(out + ch * plane) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
    } else {
#pragma unroll
      for (int j = 0; j < kCols; ++j)
        if (c0 + j < ow) out[ch * plane + j] = v[ch][j];
    }
  }
}

__global__ __launch_bounds__(kTile) void frames_to_depths_kernel(const uint16_t* __restrict__ depth_mm, const int32_t* __restrict__ ys,
                                                                 const int32_t* __restrict__ xs, float* __restrict__ depths,
                                                                 unsigned long long n_out, int H, int W, int oh, int ow) {
#pragma clang fp contract(off)
  const unsigned long long gid = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
  if (gid >= n_out) return;
  const unsigned long long rowid = gid / (unsigned)ow;             // img * oh + r
  const int c = (int)(gid - rowid * (unsigned)ow);
  const unsigned long long img = rowid / (unsigned)oh;
  const int r = (int)(rowid - img * (unsigned)oh);
  const uint16_t mm = depth_mm[((size_t)img * H + clampi(ys[r], H - 1)) * W + clampi(xs[c], W - 1)];
  const float d = (float)mm / 1000.0f;
  depths[gid] = d > 65.0f ? 0.0f : d;
}

// sizes of both entry points: positive, and a launch of fewer than 2^31 workgroups
int check_sizes(const char* who, int n, int H, int W, int oh, int ow, int per_thread, unsigned long long* n_threads,
                unsigned* blocks) {
  V3D_REQUIRE(n > 0 && H > 0 && W > 0 && oh > 0 && ow > 0, V3D_ERR_BAD_SHAPE,
              "%s: n, H, W, oh, ow must be positive (got %d, %d, %d, %d, %d)", who, n, H, W, oh, ow);
  // the kernels index with 64-bit offsets: 3 n H W source bytes must stay below 2^62 (a product of two ints fits 64 bits, the
  // third factor is checked by division), and the launch below 2^31 workgroups
  const unsigned long long hw = (unsigned long long)H * W;
  V3D_REQUIRE(hw <= ((1ull << 62) / 3) / (unsigned)n, V3D_ERR_BAD_SHAPE, "%s: n * H * W = %d * %llu frame pixels are too many", who, n, hw);
  const unsigned long long groups = ((unsigned long long)ow + per_thread - 1) / per_thread;
  const unsigned long long rows = (unsigned long long)n * oh;
  const unsigned long long max_threads = ((1ull << 31) - 1) * kTile;
  V3D_REQUIRE(rows <= max_threads / groups, V3D_ERR_BAD_SHAPE, "%s: n * oh * ow = %llu * %d outputs are too many for one launch", who,
              rows, ow);
  const unsigned long long threads = rows * groups;
  const unsigned long long nb = (threads + kTile - 1) / kTile;
  *n_threads = threads;
  *blocks = (unsigned)nb;
  return V3D_OK;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int v3d_frames_to_images_f32(const uint8_t* frames, int n, int H, int W, const int32_t* y0, const int32_t* y1,
                                        const float* wy, const int32_t* x0, const int32_t* x1, const float* wx, int oh, int ow,
                                        int quantize, float scale_rgb, const float* mean_host, const float* std_host, float* images,
                                        void* stream) {
  const char* who = "v3d_frames_to_images_f32";
  V3D_REQUIRE(frames && y0 && y1 && wy && x0 && x1 && wx && mean_host && std_host && images, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(aligned(y0, 4) && aligned(y1, 4) && aligned(wy, 4) && aligned(x0, 4) && aligned(x1, 4) && aligned(wx, 4) &&
                  aligned(images, 4),
              V3D_ERR_BAD_ARG, "%s: the tables and images must be aligned to 4 bytes", who);
  unsigned long long n_threads;
  unsigned blocks;
  const int rc = check_sizes(who, n, H, W, oh, ow, kCols, &n_threads, &blocks);
  if (rc != V3D_OK) return rc;
  ColourNorm nrm;
  nrm.scale = scale_rgb;
  V3D_REQUIRE(std::isfinite(scale_rgb) && scale_rgb != 0.f, V3D_ERR_BAD_ARG, "%s: scale_rgb = %g is zero or not finite", who, scale_rgb);
  for (int c = 0; c < 3; ++c) {
    nrm.mean[c] = mean_host[c];
    nrm.std[c] = std_host[c];
    V3D_REQUIRE(std::isfinite(nrm.mean[c]) && std::isfinite(nrm.std[c]) && nrm.std[c] != 0.f, V3D_ERR_BAD_ARG,
                "%s: mean[%d] = %g / std[%d] = %g: not finite, or a zero std", who, c, nrm.mean[c], c, nrm.std[c]);
  }
  const int groups = (ow + kCols - 1) / kCols;
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("frames_to_images", s);
    if (ow % kCols == 0 && aligned(images, 16))
      frames_to_images_kernel<true><<<blocks, kTile, 0, s>>>(frames, y0, y1, wy, x0, x1, wx, images, nrm, quantize != 0, n_threads, H, W,
                                                             oh, ow, groups);
    else
      frames_to_images_kernel<false><<<blocks, kTile, 0, s>>>(frames, y0, y1, wy, x0, x1, wx, images, nrm, quantize != 0, n_threads, H,
                                                              W, oh, ow, groups);
  }
  V3D_CHECK_LAUNCH("frames_to_images_kernel");
  return V3D_OK;
}

extern "C" int v3d_frames_to_depths_f32(const uint16_t* depth_mm, int n, int H, int W, const int32_t* ys, const int32_t* xs, int oh,
                                        int ow, float* depths, void* stream) {
  const char* who = "v3d_frames_to_depths_f32";
  V3D_REQUIRE(depth_mm && ys && xs && depths, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(aligned(depth_mm, 2) && aligned(ys, 4) && aligned(xs, 4) && aligned(depths, 4), V3D_ERR_BAD_ARG,
              "%s: depth_mm must be aligned to 2 bytes, the tables and depths to 4", who);
  unsigned long long n_out;
  unsigned blocks;
  const int rc = check_sizes(who, n, H, W, oh, ow, 1, &n_out, &blocks);
  if (rc != V3D_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("frames_to_depths", s);
    frames_to_depths_kernel<<<blocks, kTile, 0, s>>>(depth_mm, ys, xs, depths, n_out, H, W, oh, ow);
  }
  V3D_CHECK_LAUNCH("frames_to_depths_kernel");
  return V3D_OK;
}
