// The per-pixel rule of the 2D depth metrics (include/v3d.h states it under v3d_depth_metrics_2d), shared by the two kernels that
// score depth maps: csrc/depthmetrics.hip (walks the ground truth, gathers the prediction) and csrc/supervision.hip (walks the
// prediction, gathers the ground truth).  The rule exists once.
//
// Arithmetic per pixel: float64, every operation rounded on its own (no contraction of e e + S into an FMA), divisions and the
// square root are the IEEE ones; the one fp32 operation is 1 / p, because the reference's prediction is a float32 tensor there.
#ifndef V3D_DEPTH_PIXEL_H_
#define V3D_DEPTH_PIXEL_H_
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace v3d {
namespace depth2d {

struct Acc {
  double rel, diff, inv, sqrel, sq;
  int pv, m, c1, c2, c3;
};

__device__ __forceinline__ void pixel(Acc& a, double g, float pf, int valid_mode, uint8_t vbyte) {
#pragma clang fp contract(off)
  const double p = (double)pf;
  const bool pv = valid_mode == 0 ? true : valid_mode == 1 ? vbyte != 0 : (pf != 0.f && fabsf(pf) != INFINITY);   // NaN: valid
  const bool m = pv && g >= 0.5 && g < 65.0;
  a.pv += pv;
  a.m += m;
  if (m) {
    const double e = fabs(p - g), q = g + 1e-7;
    a.rel += e / q;
    a.diff += e;
    const double t = fabs((double)(1.0f / pf) - 1.0 / g);
    a.inv += fabs(t) < (double)INFINITY ? t : 0.0;                 // inf and NaN count as 0
    const double ee = e * e;
    a.sqrel += ee / q;
    a.sq += ee;
    const double r1 = p / g, r2 = g / p;                           // max(r1, r2) < x  <=>  both < x; a NaN makes it false
    a.c1 += r1 < 1.25 && r2 < 1.25;
    a.c2 += r1 < 1.5625 && r2 < 1.5625;
    a.c3 += r1 < 1.953125 && r2 < 1.953125;
  }
}

// lanes -> lane 0 of the wave, by shuffles in a fixed order
__device__ __forceinline__ void wave_reduce(Acc& a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a.rel += __shfl_down(a.rel, off);
    a.diff += __shfl_down(a.diff, off);
    a.inv += __shfl_down(a.inv, off);
    a.sqrel += __shfl_down(a.sqrel, off);
    a.sq += __shfl_down(a.sq, off);
    a.pv += __shfl_down(a.pv, off);
    a.m += __shfl_down(a.m, off);
    a.c1 += __shfl_down(a.c1, off);
    a.c2 += __shfl_down(a.c2, off);
    a.c3 += __shfl_down(a.c3, off);
  }
}

// One image's row of the nine metrics from its five sums s and five counts c over HW scored pixels.  The reference's types: the
// mask's sum is a float32 tensor, + 1e-7 is one fp32 addition; the float64 sums are divided by its widening, the fp32 counts by
// itself.
__device__ __forceinline__ void finish_row(const double* s, const int* c, int HW, double* row) {
#pragma clang fp contract(off)
  const float denom32 = (float)c[1] + 1e-7f;
  const double denom = (double)denom32;
  row[0] = (double)((float)c[0] / (float)HW);
  row[1] = s[0] / denom;
  row[2] = s[1] / denom;
  row[3] = s[2] / denom;
  row[4] = s[3] / denom;
  row[5] = sqrt(s[4] / denom);
  row[6] = (double)((float)c[2] / denom32);
  row[7] = (double)((float)c[3] / denom32);
  row[8] = (double)((float)c[4] / denom32);
}

}  // namespace depth2d
}  // namespace v3d
#endif  // V3D_DEPTH_PIXEL_H_
