// CostRegNet, conv9 + prob fused (mvsnet.py:161-162): x_reg = prob(conv0 + ReLU(BN(deconv9(u8)))), the last layers of both
// chains (costreg.hip is the map of the family).
// The 8-channel full-resolution tensor between the last deconvolution and the 1-channel prob conv (308 MB per
// 32 references, written once and read once) never leaves the CU: a workgroup owns a 4 x 8 x 28 tile of the
// prob output, computes the deconvolution on the tile + 1 halo (6 x 10 x 30) with split-bf16 MFMAs, adds the
// conv0 skip, parks the result in LDS and runs the 3x3x3x8 prob conv from there.
//
// Deconvolution as a GEMM over "cells".  ConvTranspose3d(k=3, stride 2, pad 1, output_padding 1) gives
// out[o] = sum_i in[i] w[o - 2i + 1], so per axis output 2j+1 = in[j] w[2] + in[j+1] w[0] and output 2j+2 =
// in[j+1] w[1].  Cell j therefore owns outputs (2j+1, 2j+2) and reads inputs (j, j+1); the halo'd tile starts
// at an odd output, i.e. it is exactly 3 x 5 x 15 cells.  One MFMA tile: 16 columns = the 15 cells of an x row
// (+1 idle), 16 rows = 2 x parities x 8 output channels, K = 32 = 2 x inputs x 16 input channels; the
// (z, y) parities / inputs are separate blocks, of which 9 of 16 hold weights (the 27 taps).
#include "costreg.h"
#include "phase_timing.h"
#include "weight_pack.h"

PHASE_TIMING_UNIT(v3d_debug_conv9_phase_read)

namespace v3d {
namespace {

struct C9 {
  static constexpr int TD = 4, TH = 8, TW = 28;                    // prob output tile
  static constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2;      // u9 tile with halo
  static constexpr int CZ = HD / 2, CY = HH / 2, CX = HW / 2;      // 3 x 5 x 15 cells
  static constexpr int VZ = CZ + 1, VY = CY + 1, VX = CX + 2;      // 4 x 6 x (16 + 1 idle) input voxels
  static constexpr int NVOX = VZ * VY * VX;
  static constexpr int RS = 32;                                    // u9 tile row stride in floats
  static constexpr int U9_BYTES = 8 * HD * HH * RS * 4;            // 61440: [4 channel pairs][HD][HH][RS][2]
  static constexpr int IN_BYTES = NVOX * 2 * 16 * 2;               // hi + lo, two 8-channel halves per voxel
  static constexpr int LDS_BYTES = U9_BYTES > IN_BYTES ? U9_BYTES : IN_BYTES;
  static constexpr int NCB = CZ * CY;                              // 15 cell rows = MFMA column blocks
  static constexpr int WU32 = 9 * 2 * 64 * 4;                      // weight image words
  // exact-fp32 variant (conv9_prob_kernel<true>): the input tile as [16 channels][VZ][VY][VX] floats at a channel stride of
  // FS floats (== 16 mod 64: the four k lane groups of a B fragment read four channels' rows from four different bank
  // quarters), the weight fragments as [9 blocks][2 halves][64 lanes][4 k slices] floats
  static constexpr int FS = 464, WF32 = 9 * 64 * 8;
  static_assert(FS >= NVOX && FS % 64 == 16 && (16 * FS + WF32) * 4 <= U9_BYTES, "fp32 input tile + weights share the u9 region");
};

struct C9Params {
  const float* u8;     // conv8 output in the split layout [n][2 groups][hi, lo][D/2][H/2][W/2][8 bf16]   (F32: fp32 [n, 16, D/2, H/2, W/2])
  const float* c0;     // conv0 output (skip) in the split channel-last layout [n][hi, lo][D][H][W][8 bf16]  (F32: fp32 [n, 8, D, H, W])
  const float* wbf;    // split-bf16 fragment image of the deconv weights (BN scale folded)                 (F32: fp32 fragments, C9::WF32)
  const float* bias9;  // [8] folded BN bias
  const float* wprob;  // [4 channel pairs, 27, 2]
  const float* bprob;  // [1]
  float* out;          // [n, D, H, W]
  int n, D, H, W, ntz, nty, ntx;
  int zy_order;        // tile_order(): 1 = x, z, y
  unsigned m_tx, m_t1, m_t2;   // v3d::magic_u32() of ntx and of the two tile counts divided after it (in zy_order's order)
};

// Address arithmetic (round 4).  A workgroup lives for one tile, so its prologue -- tile index -> (n, tz, ty, tx), the clamped
// addresses of 3 input slots and 16 skip half-slots per lane -- is paid per tile: written with size_t indices it was 46
// quarter-rate integer instructions (v_mad_u64_u32, v_mul_lo_u32, five v_rcp_iflag_f32 division sequences) among ~850 VALU
// instructions of a wave, as many issue slots as the prob conv's FMAs.  Now: host magic numbers for the tile index, 24-bit
// multiplies, wave-uniform row bases in SGPRs + 32-bit lane offsets (the host checks that a view's tensors stay below 4 GB).
// 8 waves per workgroup, <= 128 VGPRs: two workgroups = 16 waves per CU (round 1's 4-wave version needed 218 VGPRs, i.e.
// 8 waves per CU, and spent most of its time waiting for its own loads, barriers and LDS round trips: 0.55 -> 0.45 ms).  The weight fragments
// are parked in LDS next to the input tile (both are dead before the u9 tile overwrites them) instead of 72 registers, a
// wave owns two of the 15 cell rows in the deconvolution, and in the prob conv a lane owns two consecutive outputs so that
// the 16 lanes of a row read 16 consecutive 16-byte slots (conflict-free; the 4-outputs-per-lane mapping read at a 32-byte
// lane stride: 2-way conflicts on every read).  Accumulation orders are those of the 4-wave kernel: bit-identical output.
#ifndef V3D_C9_ABLATE
#define V3D_C9_ABLATE 0      // developer ablations (scripts/ab_build.sh): 1 no prob loop, 2 one channel pair only, 3 no MFMAs, 4 no skip loads, 5 no input loads
#endif
// F32 (round 4, the exact-fp32 chain): the same tile structure on v_mfma_f32_16x16x4_f32 -- fp32 tensors in the reference
// layout in, eight k slices of 4 per block where the split path has three bf16 products of 32 -- instead of the generic
// per-layer conv9 kernel + prob_conv_kernel, which wrote and re-read the 8-channel full-resolution tensor (0.82 + 0.30 ms).
template <bool F32>
__global__ __launch_bounds__(512, 4) void conv9_prob_kernel(C9Params p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[C9::LDS_BYTES];
  u32x4* const xh = reinterpret_cast<u32x4*>(smem);             // [NVOX][2 halves] hi slots
  u32x4* const xl = xh + C9::NVOX * 2;                          // lo slots
  u32x4* const wfr = xl + C9::NVOX * 2;                         // [9 blocks][hi, lo][64 lanes] weight fragments
  float* const xf = reinterpret_cast<float*>(smem);             // F32: [16][FS] input tile
  float* const wff = xf + 16 * C9::FS;                          // F32: [9 blocks][2 halves][64 lanes][4 k slices] weight fragments
  float* const u9s = reinterpret_cast<float*>(smem);            // [8][HD][HH][RS], reuses the input tile
  static_assert(C9::IN_BYTES + C9::WU32 * 4 <= C9::U9_BYTES, "input tile + weight fragments share the u9 region");
  constexpr int NT = 512, NCBI = 2;                             // threads, cell rows per wave (15 rows over 8 waves)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const unsigned b0 = (unsigned)v3d::xcd_contiguous_block();
  const unsigned b1 = v3d::udiv_magic(b0, (unsigned)p.ntx, p.m_tx);
  const int tx = (int)(b0 - b1 * (unsigned)p.ntx);
  int ty, tz, n;
  {
    const unsigned d1 = (unsigned)(p.zy_order ? p.ntz : p.nty), d2 = (unsigned)(p.zy_order ? p.nty : p.ntz);
    const unsigned b2 = v3d::udiv_magic(b1, d1, p.m_t1), b3 = v3d::udiv_magic(b2, d2, p.m_t2);
    const int t1 = (int)(b1 - b2 * d1), t2 = (int)(b2 - b3 * d2);
    tz = p.zy_order ? t1 : t2;
    ty = p.zy_order ? t2 : t1;
    n = (int)b3;
  }
  const int oz0 = tz * C9::TD, oy0 = ty * C9::TH, ox0 = tx * C9::TW;
  const int D2 = p.D >> 1, H2 = p.H >> 1, W2 = p.W >> 1;
  const int iz0 = (oz0 >> 1) - 1, iy0 = (oy0 >> 1) - 1, ix0 = (ox0 >> 1) - 1;
  const size_t in_plane = (size_t)D2 * H2 * W2;
  const size_t out_plane = (size_t)p.D * p.H * p.W;

  PHASE_DECL;
  // ---- global reads with clamped addresses (no branches): (a) the 4 x 6 x 16 x 16ch input tile ([n][2 groups][hi, lo]
  // [D/2][H/2][W/2] slots: 2 x 2 x 384 slots, three 16-byte copies per thread) and the weight fragments
  u32x4 pre[3], wpre[3];
  constexpr int NF = (16 * C9::VZ * C9::VY * 16 + NT - 1) / NT;      // F32: floats per thread of the 16 x 4 x 6 x 16 tile (column 16 is idle)
  constexpr int NWF = C9::WF32 / 4 / NT + 1;                        // F32: 16-byte pieces of the weight image per thread
  float pref[F32 ? NF : 1];
  u32x4 wpref[F32 ? NWF : 1];
  if constexpr (F32) {
    // rows of 16 floats: row R = (ci * VZ + vz) * VY + vy, 32 rows per pass of the workgroup
    const char* const src = reinterpret_cast<const char*>(p.u8 + (size_t)n * 16 * in_plane);
    const int vx = tid & 15;
    const int gx = ix0 + vx;
    const int xc = min(max(gx, 0), W2 - 1);
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const unsigned R = (unsigned)(tid >> 4) + 32u * i;                 // < 16 * 24 = 384
      const unsigned ci = v3d::small_div<C9::VZ * C9::VY>(R), rem = R - ci * (C9::VZ * C9::VY);
      const unsigned uz = v3d::small_div<C9::VY>(rem);
      const int gz = iz0 + (int)uz, gy = iy0 + (int)(rem - uz * C9::VY);
      const bool ok = gz >= 0 && gz < D2 && gy >= 0 && gy < H2 && gx >= 0 && gx < W2;
      const int zc = min(max(gz, 0), D2 - 1), yc = min(max(gy, 0), H2 - 1);
      const unsigned idx = __umul24(ci, (unsigned)in_plane) + __umul24(__umul24(zc, H2) + yc, W2) + xc;
      const float val = *reinterpret_cast<const float*>(src + idx * 4u);
      pref[i] = ok ? val : 0.f;
    }
    const u32x4* wq = reinterpret_cast<const u32x4*>(p.wbf);
#pragma unroll
    for (int i = 0; i < NWF; ++i) wpref[i] = wq[min(tid + NT * i, C9::WF32 / 4 - 1)];
  } else {
    const char* const src = reinterpret_cast<const char*>(reinterpret_cast<const u32x4*>(p.u8) + (size_t)n * 4 * in_plane);
    const int vx = tid & 15;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      // slot it = tid + NT * i of the [4 (group, part)][VZ][VY][16] tile: row R = it / 16 = (gp * VZ + vz) * VY + vy
      const unsigned R = (unsigned)(tid >> 4) + 32u * i;                // 32 i .. 32 i + 31
      const bool up = R >= 24u * (i + 1);                                // gp = R / 24 = i or i + 1
      const unsigned rem = R - (up ? 24u * (i + 1) : 24u * i);           // R % 24
      const unsigned uz = __umul24(rem, 43u) >> 8;                       // rem / 6 (exact below 24)
      const int vz = (int)uz, vy = (int)(rem - __umul24(uz, 6u));
      const int gz = iz0 + vz, gy = iy0 + vy, gx = ix0 + vx;
      const bool ok = gz >= 0 && gz < D2 && gy >= 0 && gy < H2 && gx >= 0 && gx < W2;
      const int zc = min(max(gz, 0), D2 - 1), yc = min(max(gy, 0), H2 - 1), xc = min(max(gx, 0), W2 - 1);
      const unsigned idx = (unsigned)in_plane * i + (up ? (unsigned)in_plane : 0u) + __umul24(__umul24(zc, H2) + yc, W2) + xc;   // < 2^28 (host check)
      const u32x4 val = V3D_C9_ABLATE == 5 ? (u32x4){1u, 2u, 3u, (unsigned)tid} : *reinterpret_cast<const u32x4*>(src + idx * 16u);
      pre[i] = ok ? val : (u32x4){0u, 0u, 0u, 0u};
    }
    const u32x4* wq = reinterpret_cast<const u32x4*>(p.wbf);
#pragma unroll
    for (int i = 0; i < 3; ++i) wpre[i] = wq[min(tid + NT * i, C9::WU32 / 4 - 1)];
  }
  __builtin_amdgcn_sched_barrier(0);
  // (b) the conv0 skip values of this lane's outputs, in flight during staging and the MFMA phase.  conv0's output is in
  // the split channel-last layout ([n][hi, lo][D][H][W] slots of 8 channels): channels cbase..cbase+3 are 8 bytes of the hi
  // slot and 8 bytes of the lo slot
  const int px = kq >> 1, cbase = 4 * (kq & 1);
  u32x2 skh[NCBI][4], skl[NCBI][4];
  float skf[F32 ? NCBI : 1][4][4];
  if constexpr (F32) {
    // fp32 [n, 8, D, H, W]: the lane's four channels are four planes apart
    const char* const skip = reinterpret_cast<const char*>(p.c0 + ((size_t)n * 8 + cbase) * out_plane);
    const int gx = ox0 - 1 + 2 * jn + px;
    const unsigned lofs = (unsigned)min(max(gx, 0), p.W - 1) * 4u;
    const unsigned cpl = (unsigned)out_plane * 4u;                       // bytes per channel plane (< 2^28, host check)
#pragma unroll
    for (int cbi = 0; cbi < NCBI; ++cbi) {
      const int cb = min(wave + 8 * cbi, C9::NCB - 1);
      const int cz = cb / C9::CY, cy = cb % C9::CY;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const int gz = oz0 - 1 + 2 * cz + (rb >> 1), gy = oy0 - 1 + 2 * cy + (rb & 1);
        const int zc = min(max(gz, 0), p.D - 1), yc = min(max(gy, 0), p.H - 1);
        const unsigned rofs = (unsigned)((zc * p.H + yc) * p.W) * 4u;      // wave-uniform
#pragma unroll
        for (int r = 0; r < 4; ++r) skf[cbi][rb][r] = *reinterpret_cast<const float*>(skip + (size_t)r * cpl + rofs + lofs);
      }
    }
  } else {
    const char* const skip = reinterpret_cast<const char*>(reinterpret_cast<const u32x2*>(p.c0) + ((size_t)n * 2 * out_plane) * 2);
    // the row (z, y) of a (cell row, rb) is wave-uniform: its base stays in SGPRs, the lane adds its x slot and channel half
    const int gx = ox0 - 1 + 2 * jn + px;
    const unsigned lofs = (unsigned)min(max(gx, 0), p.W - 1) * 16u + (unsigned)(kq & 1) * 8u;
    const unsigned lo_plane = (unsigned)out_plane * 16u;                  // hi slots -> lo slots, bytes (< 2^31, host check)
#pragma unroll
    for (int cbi = 0; cbi < NCBI; ++cbi) {
      const int cb = min(wave + 8 * cbi, C9::NCB - 1);
      const int cz = cb / C9::CY, cy = cb % C9::CY;
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const int gz = oz0 - 1 + 2 * cz + (rb >> 1), gy = oy0 - 1 + 2 * cy + (rb & 1);
        const int zc = min(max(gz, 0), p.D - 1), yc = min(max(gy, 0), p.H - 1);
        const unsigned rofs = (unsigned)((zc * p.H + yc) * p.W) * 16u;     // wave-uniform
        skh[cbi][rb] = V3D_C9_ABLATE == 4 ? (u32x2){rofs + lofs, 1u} : *reinterpret_cast<const u32x2*>(skip + rofs + lofs);
        skl[cbi][rb] = V3D_C9_ABLATE == 4 ? (u32x2){rofs + lofs, 2u} : *reinterpret_cast<const u32x2*>(skip + lo_plane + rofs + lofs);
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- stage the input tile (slot = voxel * 2 + channel half (group), hi and lo arrays) and the weight fragments ------
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const unsigned R = (unsigned)(tid >> 4) + 32u * i;
      const unsigned ci = v3d::small_div<C9::VZ * C9::VY>(R), rem = R - ci * (C9::VZ * C9::VY);      // rem = vz * VY + vy
      if (R < 16 * C9::VZ * C9::VY) xf[ci * C9::FS + rem * C9::VX + (tid & 15)] = pref[i];
    }
#pragma unroll
    for (int i = 0; i < NWF; ++i)
      if (tid + NT * i < C9::WF32 / 4) reinterpret_cast<u32x4*>(wff)[tid + NT * i] = wpref[i];
    // the idle 17th voxel of every row is read by column 15: keep it finite
    for (int i = tid; i < 16 * C9::VZ * C9::VY; i += NT) {
      const unsigned ci = v3d::small_div<C9::VZ * C9::VY>((unsigned)i), rem = (unsigned)i - ci * (C9::VZ * C9::VY);
      xf[ci * C9::FS + rem * C9::VX + 16] = 0.f;
    }
  } else {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const unsigned R = (unsigned)(tid >> 4) + 32u * i;                   // as above
    const bool up = R >= 24u * (i + 1);
    const int gp = i + (up ? 1 : 0);
    const unsigned rem = R - (up ? 24u * (i + 1) : 24u * i);             // vz * VY + vy
    const int slot = (int)(__umul24(rem, (unsigned)C9::VX) + (unsigned)(tid & 15)) * 2 + (gp >> 1);
    ((gp & 1) ? xl : xh)[slot] = pre[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (tid + NT * i < C9::WU32 / 4) wfr[tid + NT * i] = wpre[i];
  if (tid < C9::VZ * C9::VY * 2) {         // the idle 17th voxel of every row is read by column 15: keep it finite
    const int slot = ((tid >> 1) * C9::VX + 16) * 2 + (tid & 1);
    xh[slot] = (u32x4){0u, 0u, 0u, 0u};
    xl[slot] = (u32x4){0u, 0u, 0u, 0u};
  }
  }
  PHASE_MARK(0);
  __syncthreads();
  PHASE_MARK(1);

  // ---- deconvolution: wave w owns cell rows w and w + 8; weight block (tz3, ty3), tz3 = {(pz 0, dz 0), (0, 1), (1, 1)},
  // likewise ty3 -------------------------------------------------------------------------------------------------------
  f32x4 acc[NCBI][4];
#pragma unroll
  for (int i = 0; i < NCBI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cbi = 0; cbi < NCBI; ++cbi) {
    const int cb = wave + 8 * cbi;
    if (cb < C9::NCB && V3D_C9_ABLATE != 3) {
      const int cz = cb / C9::CY, cy = cb % C9::CY;
#pragma unroll
      for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          if constexpr (F32) {
            // k slice s, lane group kq: k = 4 s + kq = dx * 16 + ci  =>  dx = s >> 2, ci = 4 (s & 3) + kq
            float bv[8];
#pragma unroll
            for (int sl = 0; sl < 8; ++sl)
              bv[sl] = xf[(4 * (sl & 3) + kq) * C9::FS + ((cz + dz) * C9::VY + (cy + dy)) * C9::VX + jn + (sl >> 2)];
#pragma unroll
            for (int pz = 0; pz < 2; ++pz)
#pragma unroll
              for (int py = 0; py < 2; ++py) {
                if ((pz == 0 || dz == 1) && (py == 0 || dy == 1)) {
                  const int blk = (pz == 1 ? 2 : dz) * 3 + (py == 1 ? 2 : dy);
                  const f32x4 a0 = *reinterpret_cast<const f32x4*>(wff + ((blk * 2 + 0) * 64 + lane) * 4);
                  const f32x4 a1 = *reinterpret_cast<const f32x4*>(wff + ((blk * 2 + 1) * 64 + lane) * 4);
                  f32x4& c = acc[cbi][pz * 2 + py];
#pragma unroll
                  for (int sl = 0; sl < 8; ++sl)
                    c = __builtin_amdgcn_mfma_f32_16x16x4f32(sl < 4 ? a0[sl] : a1[sl - 4], bv[sl], c, 0, 0, 0);
                }
              }
            continue;
          }
          const int slot = (((cz + dz) * C9::VY + (cy + dy)) * C9::VX + jn + (kq >> 1)) * 2 + (kq & 1);
          const bf16x8 b_hi = __builtin_bit_cast(bf16x8, xh[slot]);
          const bf16x8 b_lo = __builtin_bit_cast(bf16x8, xl[slot]);
#pragma unroll
          for (int pz = 0; pz < 2; ++pz)
#pragma unroll
            for (int py = 0; py < 2; ++py) {
              if ((pz == 0 || dz == 1) && (py == 0 || dy == 1)) {
                const int blk = (pz == 1 ? 2 : dz) * 3 + (py == 1 ? 2 : dy);
                const bf16x8 a_hi = __builtin_bit_cast(bf16x8, wfr[(blk * 2) * 64 + lane]);
                const bf16x8 a_lo = __builtin_bit_cast(bf16x8, wfr[(blk * 2 + 1) * 64 + lane]);
                f32x4& c = acc[cbi][pz * 2 + py];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi, c, 0, 0, 0);
              }
            }
        }
    }
  }
  PHASE_MARK(2);
  __syncthreads();      // the input tile and the weight fragments are dead: their LDS becomes the u9 tile
  PHASE_MARK(3);

  // ---- BN bias + ReLU + conv0 skip -> u9 tile (zero outside the volume = the prob conv's padding) ------------
  // u9 tile layout [4 channel pairs][HD][HH][RS x][2]: a lane's channels (r, r+1) are one 8-byte write, and the
  // prob conv below multiplies both channels of a pair with one packed FMA.
  {
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = p.bias9[cbase + r];
#pragma unroll
    for (int cbi = 0; cbi < NCBI; ++cbi) {
      const int cb = wave + 8 * cbi;
      if (cb < C9::NCB && jn < C9::CX) {
        const int cz = cb / C9::CY, cy = cb % C9::CY;
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
          const int hz = 2 * cz + (rb >> 1), hy = 2 * cy + (rb & 1), hx = 2 * jn + px;
          const int gz = oz0 - 1 + hz, gy = oy0 - 1 + hy, gx = ox0 - 1 + hx;
          const bool inside = gz >= 0 && gz < p.D && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;
          float skv[4];
          if constexpr (F32) {
#pragma unroll
            for (int r = 0; r < 4; ++r) skv[r] = skf[cbi][rb][r];
          } else {
            const u32x2 sh = skh[cbi][rb], sl = skl[cbi][rb];
            skv[0] = __uint_as_float(sh.x << 16) + __uint_as_float(sl.x << 16);
            skv[1] = __uint_as_float(sh.x & 0xffff0000u) + __uint_as_float(sl.x & 0xffff0000u);
            skv[2] = __uint_as_float(sh.y << 16) + __uint_as_float(sl.y << 16);
            skv[3] = __uint_as_float(sh.y & 0xffff0000u) + __uint_as_float(sl.y & 0xffff0000u);
          }
          float val[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) val[r] = inside ? fmaxf(acc[cbi][rb][r] + bias[r], 0.f) + skv[r] : 0.f;
#pragma unroll
          for (int rp = 0; rp < 2; ++rp)
            *reinterpret_cast<f32x2*>(u9s + ((((cbase >> 1) + rp) * (C9::HD * C9::HH) + hz * C9::HH + hy) * C9::RS + hx) * 2) =
                (f32x2){val[2 * rp], val[2 * rp + 1]};
        }
      }
    }
  }
  PHASE_MARK(4);
  __syncthreads();
  PHASE_MARK(5);

  // ---- prob conv: wave = (z plane, y half), lane = (y of 4, 2 consecutive x); both channels of a pair per packed FMA --
  // (a register-ring software pipeline of the LDS reads over the 12 (pair, kz) stages measured the same 0.45 ms: this
  // phase costs 0.11 ms of the kernel, the rest is the chain loads -> staging -> MFMA -> u9 tile)
  {
    const int z = wave >> 1, y = (wave & 1) * 4 + (lane >> 4), xp = lane & 15;
    if (xp < C9::TW / 2) {
      // six accumulation chains (one pair per kz, added at the end) instead of two: a dependent v_pk_fma_f32 costs ~20 cycles
      // (measured on the retired depth-march experiment of round 4, which summed in the same order)
      f32x2 o0[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}}, o1[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
      const f32x2* wp2 = reinterpret_cast<const f32x2*>(p.wprob);       // [4 pairs][27 taps][2]
#pragma unroll 1
      for (int cp = 0; cp < (V3D_C9_ABLATE == 1 ? 0 : V3D_C9_ABLATE == 2 ? 1 : 4); ++cp) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kz = 0; kz < 3; ++kz) {
            const f32x2* row = reinterpret_cast<const f32x2*>(u9s) +
                               (cp * (C9::HD * C9::HH) + (z + kz) * C9::HH + (y + ky)) * C9::RS + 2 * xp;
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(row), q1 = *reinterpret_cast<const f32x4*>(row + 2);
            const f32x2 a0 = {q0.x, q0.y}, a1 = {q0.z, q0.w}, a2 = {q1.x, q1.y}, a3 = {q1.z, q1.w};
            const f32x2* wk = wp2 + (cp * 27 + (kz * 3 + ky) * 3);           // wave-uniform -> s_load
            const f32x2 w0 = wk[0], w1 = wk[1], w2 = wk[2];
            o0[kz] += a0 * w0; o1[kz] += a1 * w0;
            o0[kz] += a1 * w1; o1[kz] += a2 * w1;
            o0[kz] += a2 * w2; o1[kz] += a3 * w2;
          }
        }
      }
      const f32x2 s0 = (o0[0] + o0[1]) + o0[2], s1 = (o1[0] + o1[1]) + o1[2];
      const int gz = oz0 + z, gy = oy0 + y, gx = ox0 + 2 * xp;
      if (gz < p.D && gy < p.H && gx < p.W) {
        const float bsv = p.bprob[0];
        const f32x2 res = {s0.x + s0.y + bsv, s1.x + s1.y + bsv};
        float* o = p.out + ((size_t)n * out_plane + (size_t)(gz * p.H) * p.W) + (unsigned)(__umul24(gy, p.W) + gx);   // uniform base + lane offset
        if (gx + 1 < p.W && (p.W & 1) == 0) {
          *reinterpret_cast<f32x2*>(o) = res;
        } else {
          o[0] = res.x;
          if (gx + 1 < p.W) o[1] = res.y;
        }
      }
    }
  }
  PHASE_MARK(6);
  PHASE_FLUSH;
}

}  // namespace

// conv9 + skip + prob: the tile kernel (split-bf16 or exact-fp32 operands)
int launch_conv9_prob(bool f32, const v3d_costreg_weights* h, const float* u8, const float* c0, float* xreg, int n, int D, int H, int W,
                      hipStream_t s) {
  C9Params q;
  q.u8 = u8; q.c0 = c0; q.wbf = h->dev + (f32 ? h->c9f32_ofs : h->c9bf_ofs); q.bias9 = h->dev + h->bias_ofs[9];
  q.wprob = h->dev + h->prob_w2_ofs; q.bprob = h->dev + h->prob_b_ofs; q.out = xreg;
  q.n = n; q.D = D; q.H = H; q.W = W;
  q.zy_order = tile_order((W + C9::TW - 1) / C9::TW, (H + C9::TH - 1) / C9::TH);
  // 32-bit byte offsets inside one view's tensors (conv0 skip: 2 x 16 bytes per voxel / 8 fp32 planes)
  TileGrid g;
  if (const int rc = tile_grid("conv9+prob", n, D, H, W, C9::TD, C9::TH, C9::TW, q.zy_order, D, H, W, 1ll << 26, &g); rc != V3D_OK) return rc;
  q.ntz = g.ntz; q.nty = g.nty; q.ntx = g.ntx; q.m_tx = g.m_tx; q.m_t1 = g.m_t1; q.m_t2 = g.m_t2;
  {
    v3d::TimedScope ts(f32 ? "costreg_conv9_prob_f32" : "costreg_conv9_prob", s);
    // (round 6: a persistent variant -- two workgroups per CU walking their tiles, the weight fragments resident in their own
    // 18 KB of LDS, the next tile's input slots requested behind the staging barrier / the matrix phase / the u9 assembly --
    // measured 0.49-0.52 ms against the 0.43-0.45 of one workgroup per tile on the same box, wherever the prefetch sat: DESIGN.md 8.3)
    if (f32) conv9_prob_kernel<true><<<(unsigned)g.blocks, 512, 0, s>>>(q);
    else conv9_prob_kernel<false><<<(unsigned)g.blocks, 512, 0, s>>>(q);
  }
  V3D_CHECK_LAUNCH("conv9_prob_kernel");
  return V3D_OK;
}

static_assert(kConv9SplitFloats == (size_t)C9::WU32 && kConv9F32Floats == (size_t)C9::WF32, "conv9 image sizes");
// conv9 for conv9_prob_kernel, w = ConvTranspose3d weight [16][8][27].  Split-bf16 image: [block 9][hi, lo][lane 64][4 words];
// block = tz3 * 3 + ty3 with t?3 = {(parity 0, input 0), (0, 1), (1, 1)} <-> kernel tap {2, 0, 1}; rows = x parity * 8 + co,
// k = x input * 16 + ci.  fp32 image of the same GEMM for conv9_prob_kernel<true>: [block 9][half 2][lane 64][4]; k slice
// sl = half * 4 + q of v_mfma_f32_16x16x4_f32, lane group kq: k = 4 sl + kq = x input * 16 + ci
void pack_conv9(const float* w, unsigned* wb, float* wf) {
  static const int tap3[3] = {2, 0, 1};
  auto weight = [&](int blk, int m, int k) {      // row m, k = x input * 16 + ci of block blk
    const int px = m >> 3, co = m & 7, dx = k >> 4, ci = k & 15;
    const int kz = tap3[blk / 3], ky = tap3[blk % 3];
    const int kx = px == 0 ? (dx == 0 ? 2 : 0) : (dx == 1 ? 1 : -1);
    return kx < 0 ? 0.f : w[((size_t)ci * 8 + co) * 27 + kz * 9 + ky * 3 + kx];
  };
  for (int blk = 0; blk < 9; ++blk)
    for (int lane = 0; lane < 64; ++lane) {
      float v[8];
      for (int e = 0; e < 8; ++e) v[e] = weight(blk, lane & 15, (lane >> 4) * 8 + e);
      unsigned* dst = wb + (size_t)blk * 2 * kLoWords + lane * 4;
      v3d::split_bf16x8(v, dst, dst + kLoWords);
    }
  for (int blk = 0; blk < 9; ++blk)
    for (int sl = 0; sl < 8; ++sl)
      for (int lane = 0; lane < 64; ++lane)
        wf[(((size_t)blk * 2 + (sl >> 2)) * 64 + lane) * 4 + (sl & 3)] = weight(blk, lane & 15, 4 * sl + (lane >> 4));
}

// prob weights for the fused kernel, channel pairs interleaved: [4 pairs][27 taps][2]
void pack_prob(const float* prob_w, float* out) {
  for (int cp = 0; cp < 4; ++cp)
    for (int t = 0; t < 27; ++t)
      for (int e = 0; e < 2; ++e) out[((size_t)cp * 27 + t) * 2 + e] = prob_w[(cp * 2 + e) * 27 + t];
}

}  // namespace v3d
