// What the translation units of the plane-sweep warp + variance share (psv_variance.hip is the map of the family): the launch
// parameters, the tap record of a sample, the constants of the 8-pixel x 8-plane wave, the epilogue helpers, and every unit's
// launcher.  The sample geometry itself is psv_common.h's, which the backward walk (variance_backward.h) shares.
#pragma once
#include "bf16_split.h"
#include "psv_common.h"

namespace v3d {

constexpr int kMaxE = 8;     // edges per LDS pass

struct PsvParams {
  const float* featT;
  const float* K;
  const float* R;
  const float* t;
  const int* ref_img;
  const int* edge_ofs;
  const int* edge_src;
  float* var;
  const float* camp;   // [n_img][kCamStride] per-image camera block (psv_common.h, cam_block)
  int n_img, n_ref, Hf, Wf, H, W, D, h, w;
  int n_ptile;         // pixel tiles (gather kernel) / tile groups of a workgroup (reuse, window) per plane: set by the launcher
  double x_step, y_step, z_start, z_step, z_end;      // the plane-sweep grid (psv_fill_grid)
  // window kernel: launch constants the host works out once -- per wave they were two IEEE f64 divisions and three integer
  // divisions through v_rcp_iflag_f32 (round 4: ~110 of the ~2 100 VALU issue slots of a wave at cfg2)
  float rWm1, rHm1;                        // (float)(1.0 / (double)(W - 1)), (float)(1.0 / (double)(H - 1))
  unsigned m_dseg, m_ptile, m_w;           // v3d::magic_u32() of n_dseg, of n_ptile and of w (0: divide)
  // window kernel, depth walk: a wave owns its 8 pixels for `walk` consecutive chunks of kRDB planes (one depth segment; the
  // last segment of a volume may be shorter)
  int n_dchunk, walk, n_dseg;              // plane chunks per volume, chunks per segment, segments per volume
  int skip;                                // window kernel: passes whose 64 samples all miss the source image are skipped (developer option "psv_skip")
};

// zero cells behind the last bordered image (psv_prepare.hip, transpose_bordered_kernel)
__host__ __device__ constexpr int kTailCells(int Wf) { return 2 * (Wf + 2) + 16; }

struct TapInfo {      // one (pixel, plane, edge) sample, 32 bytes
  float w00, w01, w10, w11;      // nw, ne, sw, se weights: the reference's products (x1 - ix)(y1 - iy), ...
  unsigned b00;                  // byte offset of the nw cell (channel 0) in the bordered featT; ne = +CB, sw = +row, se = +row + CB
  unsigned pad[3];
};

// Bilinear taps of one sample (F.grid_sample, align_corners=True, zeros padding; mvsnet.py:209-211) on the BORDERED
// channel-last feature maps (transpose_bordered_kernel).  psv_footprint clamps the sample onto the border; a tap outside the
// image is then a zero cell and contributes exactly 0 with its true weight, as in the reference, which zeroes the tap's value.
// So there is no validity test, no per-tap clamp and one offset per sample instead of four.  CB = bytes per cell (4 C);
// first_cell = index of cell (-1, -1) of the source image.
template <unsigned CB>
__device__ __forceinline__ TapInfo make_taps(float ix, float iy, int Wf, int Hf, int first_cell) {
  const Footprint f = psv_footprint(ix, iy, Wf, Hf);      // psv_common.h: clamp, nw cell, weights
  TapInfo ti;
  ti.w00 = f.w00; ti.w01 = f.w01; ti.w10 = f.w10; ti.w11 = f.w11;
  ti.b00 = (unsigned)(first_cell + ((int)f.y0 + 1) * (Wf + 2) + (int)f.x0 + 1) * CB;
  return ti;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One sample of four channels: the blend of its footprint t00 (nw), t01 (ne), t10 (sw), t11 (se) in F.grid_sample's tap order as
// an FMA chain, ((t00 w00 + t01 w01) + t10 w10) + t11 w11, added to the sum and the sum of squares over the views.  No validity
// branch: taps outside the source image read zero cells of the border.  Every kernel blends and accumulates in this order.
__device__ __forceinline__ void psv_blend_accumulate(f32x4 t00, f32x4 t01, f32x4 t10, f32x4 t11, const TapInfo& ti, f32x4& acc_s,
                                                     f32x4& acc_q) {
  f32x4 sv = t00 * ti.w00;
  sv = __builtin_elementwise_fma(t01, (f32x4){ti.w01, ti.w01, ti.w01, ti.w01}, sv);
  sv = __builtin_elementwise_fma(t10, (f32x4){ti.w10, ti.w10, ti.w10, ti.w10}, sv);
  sv = __builtin_elementwise_fma(t11, (f32x4){ti.w11, ti.w11, ti.w11, ti.w11}, sv);
  acc_s += sv;
  acc_q = __builtin_elementwise_fma(sv, sv, acc_q);
}

// The wave of the reuse and window kernels: 8 planes x 8 pixels = 64 (pixel, plane) samples of one edge, one per lane
constexpr int kRPix = 8;      // pixels per wave
constexpr int kRDB = 8;       // depth planes per wave
#ifndef V3D_PSV_WAVES
#define V3D_PSV_WAVES 4       // waves per SIMD the two kernels are compiled for
#endif
// Waves of one workgroup only meet in the fp32 epilogue: everything else a wave exchanges through LDS is its own (LDS
// operations of a wave complete in order, so a fence that keeps the compiler from reordering them is enough).
template <int WPB>
__device__ __forceinline__ void psv_wave_sync() {
  if constexpr (WPB == 1) __syncthreads();
  else { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); }
}

// ---- epilogue: what a kernel writes from the sum s and the sum of squares q of a (voxel, channel) over the views
// The variance E[x^2] - E[x]^2 (mvsnet.py:216); mean(x) = x / clamp(count, 1), the torch_scatter mean, in the kernel's spelling.
template <class Mean>
__device__ __forceinline__ float psv_variance_value(float s, float q, Mean mean) {
  const float avg = mean(s), avg_sq = mean(q);
  return sub_rn(avg_sq, mul_rn(avg, avg));
}
// SPLIT: the variance as the regulariser's first layer consumes it (conv0z.hip, conv0z_kernel<false>): every value split
// x = hi + lo into two bf16, channel-last in 16-byte slots of 8 channels, [n_ref][4 channel groups][hi, lo][D][h][w][8] -- the
// same 4 bytes per value as fp32, and bit-identical to splitting the fp32 volume later.
// Lane (pixel, channel quad cg) of a wave with 8 lanes per pixel holds channels 4 cg .. 4 cg + 3 = one 8-byte half (cg & 1) of
// the hi slot and of the lo slot of channel group cg / 2.  Lane pairs swap halves (one DPP move per dword): the even lane
// gets the whole hi slot, the odd lane the whole lo slot -- no LDS round trip.  Every lane of the wave must call it.
__device__ __forceinline__ u32x4 psv_split_slot(const float (&v)[4], int half) {
  u32x2 hp, lp;
  split4(v[0], v[1], v[2], v[3], hp, lp);      // bf16_split.h; v_cvt_pk_bf16_f32 rounds to nearest even in hardware
  const unsigned s0 = half ? hp.x : lp.x, s1 = half ? hp.y : lp.y;             // what the partner lane stores
  const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)s0, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)s1, 0xB1, 0xf, 0xf, true);
  return half ? (u32x4){r0, r1, lp.x, lp.y} : (u32x4){hp.x, hp.y, r0, r1};
}

// ---- launchers.  Each takes the parameters by value, owns its tile size, grid and grid-size check, and sets n_ptile.
// layout: V3D_LAYOUT_REFERENCE [n_ref, C, D, h, w] fp32 | V3D_LAYOUT_SPLIT | V3D_LAYOUT_CL8 (include/v3d.h)

// psv_variance.hip: H, W, D, h, w and the plane-sweep grid of a call (the steps of psv_grid_coord / psv_plane_depth)
void psv_fill_grid(PsvParams& p, int H, int W, double depth_start, double depth_interval, int D, int h, int w);

// psv_prepare.hip: feat [n_img, C, Hf, Wf] -> featT, the bordered channel-last maps + zero tail; K, R, t -> camp, the camera blocks
int launch_psv_prepare(const float* feat, const float* K, const float* R, const float* t, int n_img, int C, int Hf, int Wf,
                       float* featT, float* camp, hipStream_t s);

// psv_fallback.hip: the gather kernel (C = 16 or 32; reference or split layout) and the reuse kernel (C = 32; reference or split)
int launch_psv_gather(PsvParams p, int C, int layout, hipStream_t s);
int launch_psv_reuse(PsvParams p, int layout, hipStream_t s);

// psv_window.hip: the window kernel (C = 32, bordered maps below 2 GB; every layout) with its walk, skip and magic numbers
int launch_psv_window(PsvParams p, int layout, hipStream_t s);

}  // namespace v3d
