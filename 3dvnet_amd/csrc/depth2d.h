// Everything the two entries that score depth maps have in common: csrc/depthmetrics.hip (v3d_depth_metrics_2d: walks the ground
// truth, gathers the prediction) and csrc/supervision.hip (v3d_depth_supervision_f32: walks the prediction, gathers the ground
// truth).  Each is a slice kernel and a finalize kernel:
//
//   slice kernel     one workgroup per slice of kSlice pixels of one walked image, the image taken as a flat H W array (walk).  A
//                    lane takes kGroup consecutive pixels per step with 16-byte loads (one for u16, two for fp32, four for fp64),
//                    gathers the other image through the two resize tables (row_src [H], col_src [W]; none = identity) and keeps
//                    NS double sums and NS 32-bit counters.  Lanes are reduced by wave shuffles, the four waves through LDS in
//                    wave order; the slice's 2 NS partials go to the workspace (reduce_store).
//   finalize kernel  one workgroup: a thread per image sums that image's slices in slice order and finalises the image's row;
//                    after a barrier one thread per column sums the rows in image order (finalize).
//
// No atomics and no scratch (build-time ISA guard).  The number of slices depends on H W alone, every order of summation is
// fixed: repeated launches and other devices give the same bits.
//
// Which lane adds which pixel, and in which order, is a function of the pixel's index in its image alone: group j of kGroup
// pixels of a slice belongs to lane j mod kThreads, the image's last group may be partial.  So every type of the walked image and
// any alignment of its base give the same bits for the same values (u16 and fp64(u16 / 1000) in particular).  A 16-byte load
// needs a 16-byte-aligned address; groups are 16, 32 or 64 bytes apart, so the whole groups of a slice are aligned together or
// not at all.  A slice that is not (the base pointer only has to be aligned to its own element: gt[1:] of odd-sized u16 images is
// 2-byte aligned) and the partial last group are read pixel by pixel, by the same lanes in the same order.
//
// Arithmetic per pixel (include/v3d.h states it under v3d_depth_metrics_2d): float64, every operation rounded on its own (no
// contraction of e e + S into an FMA), divisions and the square root are the IEEE ones; the one fp32 operation is 1 / p, because
// the reference's prediction is a float32 tensor there.
#ifndef V3D_DEPTH2D_H_
#define V3D_DEPTH2D_H_
#include <cmath>
#include <cstdint>

#include "v3d_common.h"

namespace v3d {
namespace depth2d {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlice = 8192;      // walked pixels of one image per workgroup: 38 slices of a 480 x 640 image, 10 of a 256 x 320 map
constexpr int kGroup = 8;         // consecutive pixels a lane takes per step, whatever their type: 16 bytes of u16, 32 of fp32, 64 of fp64

// What a lane keeps: the five sums and five counts of the metrics first, in the order finish_row reads them; an entry may add
// its own behind them (NS > 5).
enum { kRel, kDiff, kInv, kSqRel, kSq };      // s[]
enum { kPv, kM, kC1, kC2, kC3 };              // c[]
template <int NS>
struct Acc {
  double s[NS];
  int c[NS];
};

template <int NS>
__device__ __forceinline__ void pixel(Acc<NS>& a, double g, float pf, int valid_mode, uint8_t vbyte) {
#pragma clang fp contract(off)
  const double p = (double)pf;
  const bool pv = valid_mode == 0 ? true : valid_mode == 1 ? vbyte != 0 : (pf != 0.f && fabsf(pf) != INFINITY);   // NaN: valid
  const bool m = pv && g >= 0.5 && g < 65.0;
  a.c[kPv] += pv;
  a.c[kM] += m;
  if (m) {
    const double e = fabs(p - g), q = g + 1e-7;
    a.s[kRel] += e / q;
    a.s[kDiff] += e;
    const double t = fabs((double)(1.0f / pf) - 1.0 / g);
    a.s[kInv] += fabs(t) < (double)INFINITY ? t : 0.0;             // inf and NaN count as 0
    const double ee = e * e;
    a.s[kSqRel] += ee / q;
    a.s[kSq] += ee;
    const double r1 = p / g, r2 = g / p;                           // max(r1, r2) < x  <=>  both < x; a NaN makes it false
    a.c[kC1] += r1 < 1.25 && r2 < 1.25;
    a.c[kC2] += r1 < 1.5625 && r2 < 1.5625;
    a.c[kC3] += r1 < 1.953125 && r2 < 1.953125;
  }
}

// One image's row of the nine metrics from its five sums s and five counts c over HW scored pixels.  The reference's types: the
// mask's sum is a float32 tensor, + 1e-7 is one fp32 addition; the float64 sums are divided by its widening, the fp32 counts by
// itself.
__device__ __forceinline__ void finish_row(const double* s, const int* c, int HW, double* row) {
#pragma clang fp contract(off)
  const float denom32 = (float)c[kM] + 1e-7f;
  const double denom = (double)denom32;
  row[0] = (double)((float)c[kPv] / (float)HW);
  row[1] = s[kRel] / denom;
  row[2] = s[kDiff] / denom;
  row[3] = s[kInv] / denom;
  row[4] = s[kSqRel] / denom;
  row[5] = sqrt(s[kSq] / denom);
  row[6] = (double)((float)c[kC1] / denom32);
  row[7] = (double)((float)c[kC2] / denom32);
  row[8] = (double)((float)c[kC3] / denom32);
}

// This workgroup's slice of the flat image `walked` (W pixels per row): rule(walked value, gathered float, byte) on each of its
// pixels.  The gathered pixel of (r, c) is other[row_src[r]][col_src[c]] of the oh x ow image `other` (no tables: other[r][c]);
// the byte is bytes[pixel], 1 without bytes.
template <typename T, typename Rule>
__device__ __forceinline__ void walk(const T* __restrict__ walked, int HW, int W, int slice, const float* __restrict__ other, int oh,
                                     int ow, const int32_t* __restrict__ row_src, const int32_t* __restrict__ col_src,
                                     const uint8_t* __restrict__ bytes, Rule rule) {
  constexpr int V = 16 / (int)sizeof(T);      // elements of one 16-byte load
  struct alignas(16) Vec { T v[V]; };
  const int e0 = slice * kSlice, e1 = min(e0 + kSlice, HW);
  // a table entry outside the other image (a caller's mistake) is clamped: no read leaves the image
  auto src_row = [&](int r) { return row_src ? min(max(row_src[r], 0), oh - 1) : r; };
  auto src_col = [&](int c) { return col_src ? min(max(col_src[c], 0), ow - 1) : c; };
  // kGroup is a multiple of every V and kSlice of kGroup: all whole groups of a slice are 16-byte aligned or none is
  const bool aligned = ((uintptr_t)(walked + e0) & 15) == 0;
  const int ngroups = (e1 - e0 + kGroup - 1) / kGroup;
  for (int gi = (int)threadIdx.x; gi < ngroups; gi += kThreads) {
    const int e = e0 + gi * kGroup;
    const int cnt = min(kGroup, e1 - e);
    int r = e / W, c = e - r * W;
    const float* orow = other + (size_t)src_row(r) * ow;
    if (cnt == kGroup && aligned) {                       // the body: 16-byte loads, all gathers of the group, then the rule
      Vec wv[kGroup / V];
#pragma unroll
      for (int k = 0; k < kGroup / V; ++k) wv[k] = *reinterpret_cast<const Vec*>(walked + e + k * V);
      float of[kGroup];
      uint8_t vb[kGroup];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        of[k] = orow[src_col(c)];
        vb[k] = bytes ? bytes[e + k] : (uint8_t)1;
        if (++c == W && k + 1 < kGroup) {                 // a row (or several: W < kGroup) ends inside the group
          c = 0;
          orow = other + (size_t)src_row(++r) * ow;
        }
      }
#pragma unroll
      for (int k = 0; k < kGroup; ++k) rule(wv[k / V].v[k % V], of[k], vb[k]);
    } else {                                              // the image's last, partial group and unaligned slices: pixel by pixel
      for (int k = 0; k < cnt; ++k) {
        rule(walked[e + k], orow[src_col(c)], bytes ? bytes[e + k] : (uint8_t)1);
        if (++c == W && k + 1 < cnt) {
          c = 0;
          orow = other + (size_t)src_row(++r) * ow;
        }
      }
    }
  }
}

// lanes -> wave (shuffles in a fixed order), waves -> workgroup (LDS, wave order), the slice's partials -> the workspace
template <int NS>
__device__ __forceinline__ void reduce_store(Acc<NS>& a, double* __restrict__ part_sums, int32_t* __restrict__ part_counts) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      a.s[k] += __shfl_down(a.s[k], off);
      a.c[k] += __shfl_down(a.c[k], off);
    }
  }
  __shared__ double lds_s[kWaves][NS];
  __shared__ int lds_c[kWaves][NS];
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) lds_s[wave][k] = a.s[k], lds_c[wave][k] = a.c[k];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double s = lds_s[0][threadIdx.x];
    int cnt = lds_c[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) {
      s += lds_s[w][threadIdx.x];
      cnt += lds_c[w][threadIdx.x];
    }
    part_sums[(size_t)blockIdx.x * NS + threadIdx.x] = s;
    part_counts[(size_t)blockIdx.x * NS + threadIdx.x] = cnt;
  }
}

// The finalize kernel's body: per image its NS counts and its row of NC columns, then the NC means.  Columns 0-8 are the
// metrics; extra(s, c, row) fills an entry's own columns behind them.
template <int NS, int NC, typename Extra>
__device__ __forceinline__ void finalize(const double* __restrict__ part_sums, const int32_t* __restrict__ part_counts, int n,
                                         int slices, int HW, int32_t* __restrict__ counts, double* __restrict__ per_image,
                                         double* __restrict__ mean, Extra extra) {
#pragma clang fp contract(off)
  for (int img = (int)threadIdx.x; img < n; img += kThreads) {
    double s[NS] = {};
    int c[NS] = {};
    for (int sl = 0; sl < slices; ++sl) {
      const size_t at = ((size_t)img * slices + sl) * NS;
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        s[k] += part_sums[at + k];
        c[k] += part_counts[at + k];
      }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) counts[(size_t)img * NS + k] = c[k];
    double* row = per_image + (size_t)img * NC;
    finish_row(s, c, HW, row);
    extra(s, c, row);
  }
  __syncthreads();                       // the rows were written by this workgroup: visible to it behind the barrier
  if (threadIdx.x < NC) {
    double s = 0.;
    for (int img = 0; img < n; ++img) s += per_image[(size_t)img * NC + threadIdx.x];
    mean[threadIdx.x] = s / (double)n;
  }
}

// ---- host side: the workspace holds the slices' partial sums, then (256-byte aligned) their partial counts ----------------------
inline int slices_of(long long HW) { return (int)((HW + kSlice - 1) / kSlice); }

inline size_t counts_offset(long long blocks, int ns) { return align_up((size_t)blocks * ns * sizeof(double), 256); }

inline size_t partials_bytes(int n, int H, int W, int ns) {
  if (n <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 24)) return 0;
  const long long blocks = (long long)n * slices_of((long long)H * W);
  return counts_offset(blocks, ns) + align_up((size_t)blocks * ns * sizeof(int32_t), 256);
}

struct Partials {
  double* sums;
  int32_t* counts;
};

inline Partials carve(void* workspace, long long blocks, int ns) {
  return {(double*)workspace, (int32_t*)((char*)workspace + counts_offset(blocks, ns))};
}

}  // namespace depth2d
}  // namespace v3d
#endif  // V3D_DEPTH2D_H_
