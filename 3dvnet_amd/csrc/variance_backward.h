// The walk shared by the two backward passes of "sample every source of a reference view, take the variance over its edges":
// psv_backward.hip (the samples of a pixel are the depth planes of the sweep) and backproject_backward.hip (they are the depth
// hypotheses around the pixel's predicted depth).  Per reference view r with cnt edges, per pixel, sample k and channel:
//     x_e = bilinear sample of source e (zeros padding),  avg = sum_e x_e / cnt,  var = sum_e x_e^2 / cnt - avg^2;  given gV = dL/dvar:
//     g_e = gV * 2 * (x_e - avg) / cnt          dL/dfeat[src_e, tap, c] += w_tap * g_e   for the in-image taps.
// Nothing of size E * C * samples exists: the samples are taken again from the channel-last features.  No scratch memory either:
// every workgroup forms the camera blocks it needs in its prologue (psv_common.h: cam_block) and the accumulation target is the
// output itself.  The sample positions are the forward's, bit for bit: world_point / sample_position / psv_footprint are the same
// device functions, and the depth of a sample is spelled by the including file as its forward spells it.
//
// Work decomposition: one single-wave workgroup per (reference view, 64 / C pixels, segment of S samples); S is a compile-time
// constant.  Lane = (pixel, channel): the C lanes of a pixel read and add one contiguous 4 C-byte texel -- with C = 32 an atomic
// wave-instruction is two 128-byte texel rows, the shape global float atomics run at full rate with.
//   projection  one lane per (edge, sample, pixel): footprint cell, validity of its four taps, weights -> LDS records;
//   pass 1      every lane walks its pixel's samples for every edge: sum of x_e -> avg (S registers);
//   pass 2      the same walk again, edge by edge: g_e, and the four tap sums of the CURRENT footprint stay in registers;
//               they are flushed (up to four atomic adds) only when the footprint moves to another cell -- at far planes, or at a
//               hypothesis offset of 0.05 m, a sample moves a fraction of a texel per step, so consecutive samples share their
//               footprint.
//   In both passes the four cells of the current footprint stay in registers as well and are gathered again only when the
//   footprint moves.  More than kBwdMaxE edges per view go through LDS in chunks and are projected again in pass 2.
// Float atomics: the order in which contributions reach a texel is not fixed, so the last bits of the gradient can differ
// from call to call.
//
// What the including file supplies: a parameter struct derived from VarianceBwdParams with two device members,
//     float  sample_depth(int r, int pixel, int k, bool live) const      depth of sample k of a pixel (live: inside the problem)
//     size_t gvar_index<C>(int r, int pixel, int k, int c) const         where dL/dvar of (r, pixel, k, c) lies in gvar
// its __global__ wrapper(s) around variance_backward_walk<C, S>, and the launch.
#pragma once
#include "psv_common.h"

namespace v3d {

constexpr int kBwdMaxE = 8;     // edges per LDS pass

// One (edge, sample, pixel) record, 32 bytes.  The four cells are addressed through CLAMPED coordinates (always inside the
// source image); a tap outside the image carries weight 0 here (it adds nothing to x_e) and no validity bit (it receives
// no gradient).
struct BwdTap {
  float w00, w01, w10, w11;   // nw, ne, sw, se
  unsigned row0, row1;        // first cell of the (clamped) upper / lower row of the footprint, counted over all images
  unsigned xx;                // clamped left column | clamped right column << 16
  unsigned key;               // footprint identity: nw cell of the bordered grid ((y0 + 1) (Wf + 2) + x0 + 1) | validity << 28
};
constexpr unsigned kNoKey = 0x0fffffffu;      // no footprint: validity 0, a cell number no image has (variance_backward_limits)

// What both kernels read (variance_backward_params fills it).
struct VarianceBwdParams {
  const float* feat;          // [n_img, Hf, Wf, C]
  const float* K;
  const float* R;
  const float* t;
  const int* ref_img;
  const int* edge_ofs;
  const int* edge_src;
  const float* gvar;          // laid out as the including file's gvar_index says
  float* gfeat;               // [n_img, Hf, Wf, C], zero-filled before the launch
  int Hf, Wf, H, W, h, w;
  int n_samples;              // samples per pixel along the walked axis: planes / hypotheses
  int n_ptile, n_seg;         // pixel tiles of 64 / C pixels, segments of S samples
  double x_step, y_step;      // plane-grid steps (psv_grid_coord)
};

template <int C, int S, class Params>
__device__ __forceinline__ void variance_backward_walk(const Params& p) {
  constexpr int PPW = 64 / C;               // pixels per wave
  constexpr int ITEMS = PPW * S;            // (sample, pixel) records per edge
  constexpr int EPR = 64 / ITEMS;           // edges projected per round
  static_assert(PPW >= 1 && EPR >= 1 && EPR * ITEMS == 64, "lane roles");
  __shared__ BwdTap s_tap[kBwdMaxE * ITEMS];
  __shared__ float s_cam[1 + kBwdMaxE][kCamStride];    // [0] the reference view, [1 + e] the chunk's source views

  const int lane = threadIdx.x;
  const int c = lane % C, px = lane / C;
  int b = xcd_contiguous_block();
  const int seg = b % p.n_seg; b /= p.n_seg;            // segments fastest (see psv_fallback.hip, the reuse kernel)
  const int ptile = b % p.n_ptile;
  const int r = b / p.n_ptile;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], ne = p.edge_ofs[r + 1] - e_begin;
  if (ne == 0) return;                                  // a view without edges: var == 0 whatever the features are (wave-uniform)
  const int ref = p.ref_img[r];
  const int k0 = seg * S;

  // projection role: lane = (edge slot, sample, pixel)
  const int item = lane % ITEMS, e1 = lane / ITEMS, ks1 = item / PPW, px1 = item % PPW;
  const int gp1 = ptile * PPW + px1, k1 = k0 + ks1;
  const bool live1 = gp1 < P && k1 < p.n_samples;
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  const float rWm1 = (float)(1.0 / (double)(p.W - 1)), rHm1 = (float)(1.0 / (double)(p.H - 1));
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);
  float X = 0.f, Y = 0.f, Z = 0.f;

  // camera blocks of the chunk's source views (and, with the first chunk, of the reference view), one lane per image
  auto load_cams = [&](int ec, int nec) __attribute__((always_inline)) {
    if (lane <= nec && (lane > 0 || ec == 0)) {
      const int img = lane == 0 ? ref : p.edge_src[e_begin + ec + lane - 1];
      cam_block(p.K + img * 9, p.R + img * 9, p.t + img * 3, s_cam[lane]);
    }
  };
  auto project = [&](int ec, int nec) __attribute__((always_inline)) {
    for (int e = e1; e < nec; e += EPR) {
      float ix, iy;
      sample_position(s_cam[1 + e] + 24, X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
      // psv_footprint's clamp gives the forwards' "outside: nothing is sampled" -- a NaN or out-of-range position has no valid
      // tap with a non-zero weight
      const Footprint f = psv_footprint(ix, iy, p.Wf, p.Hf);
      const int x0 = (int)f.x0, y0 = (int)f.y0;          // in [-1, Wf] x [-1, Hf]
      const bool vx0 = x0 >= 0 && x0 < p.Wf, vx1 = x0 + 1 < p.Wf, vy0 = y0 >= 0 && y0 < p.Hf, vy1 = y0 + 1 < p.Hf;
      const unsigned valid = live1 ? (unsigned)(vx0 && vy0) | (unsigned)(vx1 && vy0) << 1 | (unsigned)(vx0 && vy1) << 2 |
                                         (unsigned)(vx1 && vy1) << 3
                                   : 0u;
      const int x0c = min(max(x0, 0), p.Wf - 1), x1c = min(x0 + 1, p.Wf - 1);
      const int y0c = min(max(y0, 0), p.Hf - 1), y1c = min(y0 + 1, p.Hf - 1);
      const unsigned img_row = (unsigned)p.edge_src[e_begin + ec + e] * (unsigned)p.Hf;
      BwdTap ti;
      ti.w00 = (valid & 1u) ? f.w00 : 0.f; ti.w01 = (valid & 2u) ? f.w01 : 0.f;
      ti.w10 = (valid & 4u) ? f.w10 : 0.f; ti.w11 = (valid & 8u) ? f.w11 : 0.f;
      ti.row0 = (img_row + (unsigned)y0c) * (unsigned)p.Wf;
      ti.row1 = (img_row + (unsigned)y1c) * (unsigned)p.Wf;
      ti.xx = (unsigned)x0c | (unsigned)x1c << 16;
      ti.key = (unsigned)((y0 + 1) * (p.Wf + 2) + x0 + 1) | valid << 28;
      s_tap[e * ITEMS + item] = ti;
    }
  };
  // The four cells of a footprint, this lane's channel.  Both passes keep them in registers while the walk along the sample axis
  // stays in one footprint and load them again only when it moves on (as the forward's plane-reuse kernel does): the
  // vector-memory path is charged per wave INSTRUCTION, and four 4-byte gathers per sample were what bounded
  // this kernel -- on 4 of 5 planes the footprint is the previous plane's.
  struct Cells { float v00, v01, v10, v11; };
  auto gather = [&](const BwdTap& ti) __attribute__((always_inline)) {
    const unsigned x0c = ti.xx & 0xffffu, x1c = ti.xx >> 16;
    return Cells{p.feat[(size_t)(ti.row0 + x0c) * C + c], p.feat[(size_t)(ti.row0 + x1c) * C + c],
                 p.feat[(size_t)(ti.row1 + x0c) * C + c], p.feat[(size_t)(ti.row1 + x1c) * C + c]};
  };
  // x_e: F.grid_sample's tap order as an FMA chain, as in the forward kernels
  auto blend = [&](const Cells& v, const BwdTap& ti) __attribute__((always_inline)) {
    float s = mul_rn(v.v00, ti.w00);
    s = __builtin_fmaf(v.v01, ti.w01, s);
    s = __builtin_fmaf(v.v10, ti.w10, s);
    return __builtin_fmaf(v.v11, ti.w11, s);
  };

  // ---- pass 1: sum of the samples over the edges, per sample of the segment ------------------------------------
  float avg[S];
#pragma unroll
  for (int k = 0; k < S; ++k) avg[k] = 0.f;
  for (int ec = 0; ec < ne; ec += kBwdMaxE) {
    const int nec = min(kBwdMaxE, ne - ec);
    __syncthreads();                       // the previous chunk's records and camera blocks are read
    load_cams(ec, nec);
    __syncthreads();
    if (ec == 0) {
      const int gy = gp1 / p.w, gx = gp1 % p.w;
      world_point(s_cam[0], psv_grid_coord(gx, p.w, p.W, p.x_step), psv_grid_coord(gy, p.h, p.H, p.y_step),
                  p.sample_depth(r, gp1, k1, live1), X, Y, Z);
    }
    project(ec, nec);
    __syncthreads();
    for (int e = 0; e < nec; ++e) {
      unsigned key = kNoKey;
      Cells v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const BwdTap ti = s_tap[e * ITEMS + k * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          v = gather(ti);
          key = ti.key;
        }
        avg[k] = add_rn(avg[k], blend(v, ti));
        // Finish this sample before the next one starts: the empty statement pins the sum here and, as a memory barrier, keeps
        // the next sample's record read and gather below it (the compiler otherwise reads the records of all S samples
        // first and blends last, 12 registers per sample: 182 VGPRs, 2 waves per SIMD, with the 16 planes of the sweep)
        asm volatile("" : "+v"(avg[k]) : : "memory");
      }
    }
  }

  // ---- avg, and gV * 2 / cnt of this lane's samples ------------------------------------------------------------
  const float cnt = (float)ne;
  const float two_over_cnt = 2.f / cnt;
  const int gp = ptile * PPW + px;
  float gs[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    avg[k] = avg[k] / cnt;
    const int ks = k0 + k;
    gs[k] = (gp < P && ks < p.n_samples) ? mul_rn(p.gvar[p.template gvar_index<C>(r, gp, ks, c)], two_over_cnt) : 0.f;
  }

  // ---- pass 2: g_e, tap sums of the current footprint in registers, atomic adds when the footprint moves ----
  const bool one_chunk = ne <= kBwdMaxE;   // the records of pass 1 are still in LDS
  for (int ec = 0; ec < ne; ec += kBwdMaxE) {
    const int nec = min(kBwdMaxE, ne - ec);
    if (!one_chunk) {
      __syncthreads();
      load_cams(ec, nec);
      __syncthreads();
      project(ec, nec);
      __syncthreads();
    }
    for (int e = 0; e < nec; ++e) {
      unsigned key = kNoKey, row0 = 0, row1 = 0, xx = 0;
      float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
      auto flush = [&]() __attribute__((always_inline)) {
        const unsigned x0c = xx & 0xffffu, x1c = xx >> 16;
        if (key & (1u << 28)) atomicAdd(p.gfeat + (size_t)(row0 + x0c) * C + c, a00);
        if (key & (2u << 28)) atomicAdd(p.gfeat + (size_t)(row0 + x1c) * C + c, a01);
        if (key & (4u << 28)) atomicAdd(p.gfeat + (size_t)(row1 + x0c) * C + c, a10);
        if (key & (8u << 28)) atomicAdd(p.gfeat + (size_t)(row1 + x1c) * C + c, a11);
      };
      Cells v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const BwdTap ti = s_tap[e * ITEMS + k * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          flush();
          key = ti.key; row0 = ti.row0; row1 = ti.row1; xx = ti.xx;
          a00 = a01 = a10 = a11 = 0.f;
          v = gather(ti);
        }
        const float g = mul_rn(sub_rn(blend(v, ti), avg[k]), gs[k]);
        a00 = __builtin_fmaf(ti.w00, g, a00);
        a01 = __builtin_fmaf(ti.w01, g, a01);
        a10 = __builtin_fmaf(ti.w10, g, a10);
        a11 = __builtin_fmaf(ti.w11, g, a11);
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11) : : "memory");   // one sample after the other, as in pass 1
      }
      flush();
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// The limits of the walk, reported in this order under the entry point's name `fn`: the kernel instances (C), the image size,
// the shape (`axis_ok`: the entry point's own condition on its sample axis), then what the tap records can hold -- 16-bit
// columns, 28-bit cell numbers of the bordered grid, 32-bit cell and element numbers over all images.
inline int variance_backward_limits(const char* fn, int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W, int h,
                                    int w, bool axis_ok) {
  V3D_REQUIRE(C == 32 || C == 16, V3D_ERR_UNSUPPORTED, "%s: C=%d unsupported (16 or 32)", fn, C);
  V3D_REQUIRE(W <= (1 << 20) && H <= (1 << 20), V3D_ERR_BAD_SHAPE, "%s: image size out of range", fn);
  V3D_REQUIRE(n_img > 0 && n_ref > 0 && n_edges >= 0 && Hf > 0 && Wf > 0 && H > 1 && W > 1 && h > 0 && w > 0 && axis_ok,
              V3D_ERR_BAD_SHAPE, "%s: bad shape", fn);
  V3D_REQUIRE(Hf < 32760 && Wf < 32760 && (long long)(Hf + 2) * (Wf + 2) < (long long)kNoKey, V3D_ERR_BAD_SHAPE,
              "%s: feature maps too large (32759 cells per axis, 2^28 per image)", fn);
  V3D_REQUIRE((long long)n_img * Hf * Wf * C < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: feature stack of 2^31 elements or more", fn);
  return V3D_OK;
}

// The geometry of a launch over `n_samples` samples per pixel in segments of `seg_len` -> the number of workgroups.
inline long long variance_backward_geometry(VarianceBwdParams& p, int n_ref, int C, int Hf, int Wf, int H, int W, int h, int w,
                                            int n_samples, int seg_len) {
  p.Hf = Hf; p.Wf = Wf; p.H = H; p.W = W; p.h = h; p.w = w;
  p.n_samples = n_samples;
  const int ppw = 64 / C;
  p.n_ptile = (int)(((long long)h * w + ppw - 1) / ppw);
  p.n_seg = (n_samples + seg_len - 1) / seg_len;
  p.x_step = w > 1 ? (double)(W - 1) / (double)(w - 1) : 0.0;
  p.y_step = h > 1 ? (double)(H - 1) / (double)(h - 1) : 0.0;
  return (long long)n_ref * p.n_ptile * p.n_seg;
}

// Output contract of both entry points: they zero-fill their accumulation target themselves.
inline hipError_t variance_backward_zero_fill(float* grad_feat_cl, int n_img, int Hf, int Wf, int C, hipStream_t s) {
  return hipMemsetAsync(grad_feat_cl, 0, (size_t)n_img * Hf * Wf * C * sizeof(float), s);
}

}  // namespace v3d
