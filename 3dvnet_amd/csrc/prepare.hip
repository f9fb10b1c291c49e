// Raw scenes -> prepared scene folders, the pixel half (data_preprocess/preprocess_scannet.py:36-70, preprocess_icl_nuim.py:181-185,
// preprocess_tum_rgbd.py:177-180): the registration of a colour frame into the depth camera and the depth-unit conversion.
//
//   register_colour_kernel   uint8 [n, Hc, Wc, 3] (interleaved, channel order as stored) -> uint8 [n, h, w, 3]: the reference's
//                            nearest grid_sample through the homography K_color K_depth^-1.  One thread per four consecutive
//                            output pixels of one row of one image, 12 bytes: each pixel's three bytes are read with byte loads
//                            and the twelve leave as three dword stores, consecutive across the wave.  Where the rows of the
//                            output are not 4-byte aligned (w % 4 != 0, or a base that is not) the same thread stores byte by
//                            byte and the last thread of a row stops at w.
//   lut_u16_kernel           out[i] = lut[in[i]] over uint16: eight elements per thread as one 16-byte load and one 16-byte
//                            store where `in` and `out` are 16-byte aligned (the thread that holds the ragged tail goes element
//                            by element); one element per thread otherwise.  The kernel holds no arithmetic: the 65 536-entry
//                            table is the reference's own NumPy expression, evaluated on the host (3dvnet_amd/preprocess.py).
//
// A sample outside the colour frame, or a coordinate that is not finite, gives three zero bytes and reads nothing, so no
// homography makes the kernel read outside `colour`.  No LDS, no atomics, no workspace, no scratch (build-time ISA guard); nothing
// depends on scheduling, so repeated launches are bit-identical.  Offsets are 64-bit throughout.
//
// Arithmetic of a sample position (include/v3d.h states it): fp32, every operation rounded on its own, no fused multiply-add, IEEE
// divisions.
#include <cmath>
#include <cstdint>

#include "v3d_common.h"

namespace {

constexpr int kTile = 256;    // threads per workgroup
constexpr int kCols = 4;      // output pixels per thread of the registration kernel
constexpr int kVec = 8;       // uint16 elements per thread of the vector path of the lut kernel

struct Homography {
  float m[9];                 // row major
  float half_w, half_h;       // Wc / 2, Hc / 2: the reference's normalisers
  float scale_x, scale_y;     // (Wc - 1) / 2, (Hc - 1) / 2: grid_sample's un-normalisation with align_corners
};

// one row of the homography applied to (x, y, 1): ((a x + b y) + c), each operation rounded
__device__ __forceinline__ float row_rn(float a, float b, float c, float x, float y) {
#pragma clang fp contract(off)
  const float p = a * x;
  const float q = b * y;
  const float s = p + q;
  return s + c;
}

// the source pixel of output pixel (x, y): true and (*jx, *jy) inside the frame, or false
__device__ __forceinline__ bool source_pixel(const Homography& hm, int x, int y, int Hc, int Wc, int* jx, int* jy) {
#pragma clang fp contract(off)
  const float xf = (float)x, yf = (float)y;
  float u = row_rn(hm.m[0], hm.m[1], hm.m[2], xf, yf);
  float v = row_rn(hm.m[3], hm.m[4], hm.m[5], xf, yf);
  float d = row_rn(hm.m[6], hm.m[7], hm.m[8], xf, yf);
  d = d + 1e-8f;
  u = u / d;
  v = v / d;
  const float gx = (u - hm.half_w) / hm.half_w;
  const float gy = (v - hm.half_h) / hm.half_h;
  const float ix = (gx + 1.0f) * hm.scale_x;
  const float iy = (gy + 1.0f) * hm.scale_y;
  const float fx = rintf(ix), fy = rintf(iy);                     // half to even
  // NaN and the infinities fail the comparisons; -0.0 is column / row 0
  if (!(fx >= 0.0f && fx < 2147483648.0f && fy >= 0.0f && fy < 2147483648.0f)) return false;
  const int cx = (int)fx, cy = (int)fy;
  if (cx >= Wc || cy >= Hc) return false;
  *jx = cx;
  *jy = cy;
  return true;
}

// VEC: every output row starts on a 4-byte boundary and w % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(kTile) void register_colour_kernel(const uint8_t* __restrict__ colour, uint8_t* __restrict__ out,
                                                                Homography hm, unsigned long long n_threads, int Hc, int Wc, int h,
                                                                int w, int groups) {
  const unsigned long long gid = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
  if (gid >= n_threads) return;
  const unsigned long long rowid = gid / (unsigned)groups;         // img * h + y
  const int c0 = (int)(gid - rowid * (unsigned)groups) * kCols;
  const unsigned long long img = rowid / (unsigned)h;
  const int y = (int)(rowid - img * (unsigned)h);
  const uint8_t* frame = colour + (size_t)img * Hc * Wc * 3;
  uint32_t px[kCols];                                               // b0 | b1 << 8 | b2 << 16 of each pixel
#pragma unroll
  for (int j = 0; j < kCols; ++j) {
    const int x = VEC ? c0 + j : min(c0 + j, w - 1);               // a ragged last thread repeats the last column and drops it below
    int jx, jy;
    px[j] = 0;
    if (source_pixel(hm, x, y, Hc, Wc, &jx, &jy)) {
      const uint8_t* p = frame + ((size_t)jy * Wc + jx) * 3;
      px[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
  }
  uint8_t* dst = out + ((size_t)rowid * w + c0) * 3;
  if (VEC) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
    d4[0] = px[0] | (px[1] << 24);
    d4[1] = (px[1] >> 8) | (px[2] << 16);
    d4[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int j = 0; j < kCols; ++j)
      if (c0 + j < w) {
        dst[3 * j + 0] = (uint8_t)px[j];
        dst[3 * j + 1] = (uint8_t)(px[j] >> 8);
        dst[3 * j + 2] = (uint8_t)(px[j] >> 16);
      }
  }
}

// VEC: in and out are 16-byte aligned; thread t holds elements [8 t, 8 t + 8)
template <bool VEC>
__global__ __launch_bounds__(kTile) void lut_u16_kernel(const uint16_t* __restrict__ in, const uint16_t* __restrict__ lut,
                                                        uint16_t* __restrict__ out, unsigned long long n_elems) {
  const unsigned long long gid = (unsigned long long)blockIdx.x * kTile + threadIdx.x;
  if (!VEC) {
    if (gid < n_elems) out[gid] = lut[in[gid]];
    return;
  }
  const unsigned long long first = gid * kVec;
  if (first >= n_elems) return;
  if (first + kVec <= n_elems) {
    const uint4 a = *reinterpret_cast<const uint4*>(in + first);
    const uint32_t src[4] = {a.x, a.y, a.z, a.w};
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (uint32_t)lut[src[k] & 0xFFFFu] | ((uint32_t)lut[src[k] >> 16] << 16);
    *reinterpret_cast<uint4*>(out + first) = make_uint4(r[0], r[1], r[2], r[3]);
  } else {
    for (unsigned long long i = first; i < n_elems; ++i) out[i] = lut[in[i]];
  }
}

// sizes of the registration (the rule of csrc/frames.hip, restated): positive, and a launch of fewer than 2^31 workgroups
int check_sizes(const char* who, int n, int Hc, int Wc, int h, int w, unsigned long long* n_threads, unsigned* blocks) {
  V3D_REQUIRE(n > 0 && Hc > 0 && Wc > 0 && h > 0 && w > 0, V3D_ERR_BAD_SHAPE,
              "%s: n, Hc, Wc, h, w must be positive (got %d, %d, %d, %d, %d)", who, n, Hc, Wc, h, w);
  // the kernel indexes with 64-bit offsets: 3 n Hc Wc source bytes must stay below 2^62 (a product of two ints fits 64 bits, the
  // third factor is checked by division), and the launch below 2^31 workgroups
  const unsigned long long hw = (unsigned long long)Hc * Wc;
  V3D_REQUIRE(hw <= ((1ull << 62) / 3) / (unsigned)n, V3D_ERR_BAD_SHAPE, "%s: n * Hc * Wc = %d * %llu frame pixels are too many", who, n,
              hw);
  const unsigned long long groups = ((unsigned long long)w + kCols - 1) / kCols;
  const unsigned long long rows = (unsigned long long)n * h;
  const unsigned long long max_threads = ((1ull << 31) - 1) * kTile;
  V3D_REQUIRE(rows <= max_threads / groups, V3D_ERR_BAD_SHAPE, "%s: n * h * w = %llu * %d outputs are too many for one launch", who, rows,
              w);
  const unsigned long long threads = rows * groups;
  *n_threads = threads;
  *blocks = (unsigned)((threads + kTile - 1) / kTile);
  return V3D_OK;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int v3d_register_colour_u8(const uint8_t* colour, int n, int Hc, int Wc, const float* homography_host, int h, int w,
                                      uint8_t* out, void* stream) {
  const char* who = "v3d_register_colour_u8";
  V3D_REQUIRE(colour && homography_host && out, V3D_ERR_BAD_ARG, "%s: null argument", who);
  unsigned long long n_threads;
  unsigned blocks;
  const int rc = check_sizes(who, n, Hc, Wc, h, w, &n_threads, &blocks);
  if (rc != V3D_OK) return rc;
  Homography hm;
  for (int k = 0; k < 9; ++k) hm.m[k] = homography_host[k];       // any value: a non-finite coordinate is a pixel outside the frame
  hm.half_w = (float)((double)Wc / 2.0);
  hm.half_h = (float)((double)Hc / 2.0);
  hm.scale_x = (float)(Wc - 1) / 2.0f;
  hm.scale_y = (float)(Hc - 1) / 2.0f;
  const int groups = (w + kCols - 1) / kCols;
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("register_colour", s);
    if (w % kCols == 0 && aligned(out, 4))
      register_colour_kernel<true><<<blocks, kTile, 0, s>>>(colour, out, hm, n_threads, Hc, Wc, h, w, groups);
    else
      register_colour_kernel<false><<<blocks, kTile, 0, s>>>(colour, out, hm, n_threads, Hc, Wc, h, w, groups);
  }
  V3D_CHECK_LAUNCH("register_colour_kernel");
  return V3D_OK;
}

extern "C" int v3d_lut_u16(const uint16_t* in, size_t n_elems, const uint16_t* lut, uint16_t* out, void* stream) {
  const char* who = "v3d_lut_u16";
  V3D_REQUIRE(in && lut && out, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(aligned(in, 2) && aligned(lut, 2) && aligned(out, 2), V3D_ERR_BAD_ARG, "%s: in, lut and out must be aligned to 2 bytes", who);
  V3D_REQUIRE(n_elems > 0, V3D_ERR_BAD_SHAPE, "%s: n_elems must be positive", who);
  const bool vec = aligned(in, 16) && aligned(out, 16);
  const unsigned long long per_block = (unsigned long long)kTile * (vec ? kVec : 1);
  const unsigned long long nb = ((unsigned long long)n_elems + per_block - 1) / per_block;
  V3D_REQUIRE(nb < (1ull << 31), V3D_ERR_BAD_SHAPE, "%s: n_elems = %llu are too many for one launch (%llu workgroups)", who,
              (unsigned long long)n_elems, nb);
  hipStream_t s = (hipStream_t)stream;
  {
    v3d::TimedScope ts("lut_u16", s);
    if (vec)
      lut_u16_kernel<true><<<(unsigned)nb, kTile, 0, s>>>(in, lut, out, n_elems);
    else
      lut_u16_kernel<false><<<(unsigned)nb, kTile, 0, s>>>(in, lut, out, n_elems);
  }
  V3D_CHECK_LAUNCH("lut_u16_kernel");
  return V3D_OK;
}
