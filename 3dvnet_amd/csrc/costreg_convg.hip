// CostRegNet, conv1..conv8 on split-bf16 matrix cores (the chain with V3D_PRECISION_SPLIT_BF16 and the per-layer entry point
// v3d_costreg_layer_split_f32; costreg.hip is the map of the family): convg_bf16x2_kernel (conv1..conv6), deconvg_bf16x2_kernel
// (conv7, conv8), their weight images, and the encoder of the layout they read.
//
// The stride-1 / stride-2 layers behind conv0 read their input in the split channel-last layout ([n][CIN/8 groups]
// [hi, lo][D][H][W] 16-byte slots of 8 channels), so staging is plain 16-byte copies.  One workgroup = one output tile
// x 16 output channels (blockIdx.y picks the channel group).  The input channels are consumed 8 at a time: a chunk's
// halo'd tile and its 9 (kz, ky) weight fragments sit in LDS while the next chunk is already in registers.  MFMA
// tile: 16 rows = output channels, 16 columns = one output x row of 14 (or two rows of 8 on the coarsest level),
// K = 32 = 4 x taps x 8 channels (tap 3 carries zero weights).  Wave w owns output row(s) y of every plane of the
// tile; an input row read from LDS feeds every plane it contributes to.  Output: fp32 [n, COUT, D, H, W] (for the
// per-layer kernels that still follow), the split layout (for the next layer of this kind), or both.
#include "costreg.h"
#include "phase_timing.h"
#include "weight_pack.h"

PHASE_TIMING_UNIT(v3d_debug_convg_phase_read)

namespace v3d {
namespace {

template <int CIN_, int COUT_, int STRIDE_, int WB_, int OUT_>
struct CG {
  static constexpr int CIN = CIN_, COUT = COUT_, S = STRIDE_, WB = WB_, OUT = OUT_;
  static constexpr int NCH = CIN / 8, NCG = COUT / 16;
  static constexpr int NRB = 16 / WB;                                  // output rows per MFMA column block
#ifndef V3D_CG_TD_S1
#define V3D_CG_TD_S1 4       // output planes per tile, stride-1 layers at 14-wide rows (developer A/B)
#endif
#ifndef V3D_CG_TD_S2
#define V3D_CG_TD_S2 3       // ... stride-2 layers (2 -> 3: conv1 0.207 -> 0.186 ms, conv3 0.116 -> 0.103; 4 leaves one workgroup per CU: 0.255)
#endif
  static constexpr int TD = WB != 14 ? (S == 2 ? 2 : 4) : S == 2 ? V3D_CG_TD_S2 : V3D_CG_TD_S1, TH = 4 * NRB, TW = WB;
  static constexpr int NKZ = 3;                                     // z taps
  static constexpr int ID = S * (TD - 1) + 3, IH = S * (TH - 1) + 3, IW = S * (TW - 1) + 3;
  static constexpr int NVOX = ID * IH * IW, NVOXP = NVOX + 8;         // idle lanes read a few slots past a row
  static constexpr int WQ = NKZ * 3 * 2 * 64;                          // 16-byte words of one chunk's weight image
  static constexpr int NVO = TD * TH * TW;
  static constexpr int LPR = IW <= 16 ? 16 : 32, RPI = 256 / LPR;      // staging: lanes per row, rows per iteration
  static constexpr int NROWS = 2 * ID * IH, NIT = (NROWS + RPI - 1) / RPI;
  static constexpr int NWIT = (WQ + 255) / 256;
  static constexpr size_t LDS_BYTES = (size_t)(2 * NVOXP + WQ) * 16;
  // Only the single-chunk layer (conv1) walks several items per workgroup: with one tile per workgroup it had no prefetch
  // at all (0.26 -> 0.22 ms).  On the multi-chunk layers the staging registers of the next item, live across the epilogue,
  // cost a workgroup per CU (conv2: 138 -> 195 VGPRs, 0.20 -> 0.25 ms), so they keep one item per workgroup.
  static constexpr bool PERSIST = NCH == 1;
  static constexpr int OCC = 2;      // (cutting conv2 / conv6 to 128 VGPRs for a fourth workgroup per CU: no gain / slower)
  static_assert(CIN % 8 == 0 && COUT % 16 == 0 && (WB == 14 || WB == 8), "shape");
  // (the output staging starts at the LDS base: behind the last barrier the weight fragments are as dead as the input tile)
  static_assert((size_t)NVO * 64 <= LDS_BYTES, "split output staging fits in the workgroup's LDS");
  static_assert((size_t)16 * (NVO + 2) * 4 <= LDS_BYTES, "fp32 output staging fits in the workgroup's LDS");
  static_assert((NROWS + RPI) * ID * IH < (1 << 20) && 4 * NVO * NVO < (1 << 20), "v3d::small_div ranges of the staging / output index");
};

struct ConvGParams {
  const void* in;      // split layout, CIN / 8 groups
  const void* wp;      // [NCG][NCH][9][hi, lo][64 lanes][4 words]
  const float* bias;   // [COUT]
  float* out_f32;      // [n, COUT, Do, Ho, Wo] or null
  void* out_split;     // split layout, COUT / 8 groups, or null
  int n, Di, Hi, Wi, Do, Ho, Wo, ntz, nty, ntx;
  unsigned m_tx, m_ty, m_tz;   // v3d::magic_u32() of ntx, nty, ntz for the item index (0: divide)
};

// PERSISTENT: the grid is the number of workgroups the chip holds; a workgroup walks (tile, output channel group) items
// first + i, first + i + G, ... of its XCD's contiguous run (v3d::xcd_tile_walk; the channel group is the fastest index, so
// the workgroups that read the same input tile run side by side).  These layers have 1 to 8 chunks per tile: with one tile
// per workgroup, conv1 (one chunk) had no prefetch at all -- load, wait, compute, store, exit.  Where C::PERSIST is set the
// first chunk of the next item is requested before the MFMAs of the current item's last chunk; elsewhere the walk has one
// item per workgroup.
// `bias_r` = p.bias as a __restrict__ kernel argument: read inside the item loop after the previous item's stores, it can
// only stay a scalar load if the compiler can exclude that the outputs alias it.
template <class C>
__global__ __launch_bounds__(256, C::OCC) void convg_bf16x2_kernel(ConvGParams p, const float* __restrict__ bias_r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* const xs = reinterpret_cast<u32x4*>(smem);                 // [hi, lo][NVOXP] slots of the current chunk
  u32x4* const wq = xs + 2 * C::NVOXP;                              // [9][hi, lo][64] weight fragments
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const size_t in_plane = (size_t)p.Di * p.Hi * p.Wi;
  const size_t out_plane = (size_t)p.Do * p.Ho * p.Wo;

  struct Item { int cg, n, oz0, oy0, ox0; };
  auto decode = [&](int t) __attribute__((always_inline)) {      // (wave-uniform: host magic numbers keep it on the scalar unit)
    Item q;
    const unsigned t0 = (unsigned)t / C::NCG;
    q.cg = (int)((unsigned)t - t0 * C::NCG);
    const unsigned t1 = v3d::udiv_magic(t0, (unsigned)p.ntx, p.m_tx), t2 = v3d::udiv_magic(t1, (unsigned)p.nty, p.m_ty);
    const unsigned t3 = v3d::udiv_magic(t2, (unsigned)p.ntz, p.m_tz);
    q.ox0 = (int)(t0 - t1 * (unsigned)p.ntx) * C::TW;
    q.oy0 = (int)(t1 - t2 * (unsigned)p.nty) * C::TH;
    q.oz0 = (int)(t2 - t3 * (unsigned)p.ntz) * C::TD;
    q.n = (int)t3;
    return q;
  };
  const v3d::TileWalk walk = v3d::xcd_tile_walk(p.n * p.ntz * p.nty * p.ntx * C::NCG);
  if (walk.t >= walk.end) return;

  // ---- staging: chunk c = input channel group c (hi rows then lo rows) + its weight image -----------------------
  const int lrow = tid / C::LPR, lx = tid % C::LPR;
  const bool xok = lx < C::IW;
  u32x4 pre[C::NIT], wreg[C::NWIT];
  constexpr bool XPRE = C::PERSIST;
  auto issue = [&](const Item& q, int chunk) __attribute__((always_inline)) {
    const int iz0 = C::S * q.oz0 - 1, iy0 = C::S * q.oy0 - 1, sgx = C::S * q.ox0 - 1 + lx;
    const bool xin = xok && sgx >= 0 && sgx < p.Wi;
    const int sxc = min(max(sgx, 0), p.Wi - 1);
    // (wave-uniform 64-bit base of the chunk's hi plane + a 32-bit lane offset built from 24-bit multiplies: with size_t
    // indices every row cost a v_mad_u64_u32 and two v_mul_lo_u32, quarter-rate instructions; the host checks the range)
    const char* const ins = reinterpret_cast<const char*>(reinterpret_cast<const u32x4*>(p.in) +
                                                          ((size_t)q.n * C::NCH + chunk) * 2 * in_plane);
    const u32x4* const wg = reinterpret_cast<const u32x4*>(p.wp) + (size_t)q.cg * C::NCH * C::WQ;
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const unsigned rr = (unsigned)(it * C::RPI + lrow);
      const unsigned part = v3d::small_div<C::ID * C::IH>(rr), rem = rr - part * (C::ID * C::IH);
      const unsigned rz = v3d::small_div<C::IH>(rem), ry = rem - rz * C::IH;
      const int gz = iz0 + (int)rz, gy = iy0 + (int)ry;
      const bool ok = rr < C::NROWS && xin && gz >= 0 && gz < p.Di && gy >= 0 && gy < p.Hi;
      const int zc = min(max(gz, 0), p.Di - 1), yc = min(max(gy, 0), p.Hi - 1);
      const unsigned idx = (part ? (unsigned)in_plane : 0u) + __umul24(__umul24(zc, p.Hi) + yc, p.Wi) + sxc;
      const u32x4 v = *reinterpret_cast<const u32x4*>(ins + idx * 16u);
      pre[it] = ok ? v : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i)
      wreg[i] = (i * 256 + tid < C::WQ) ? wg[(size_t)chunk * C::WQ + i * 256 + tid] : (u32x4){0u, 0u, 0u, 0u};
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const unsigned rr = (unsigned)(it * C::RPI + lrow);
      const unsigned part = v3d::small_div<C::ID * C::IH>(rr), rem = rr - part * (C::ID * C::IH);
      if (rr < C::NROWS && xok) xs[part * C::NVOXP + rem * C::IW + lx] = pre[it];
    }
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i)
      if (i * 256 + tid < C::WQ) wq[i * 256 + tid] = wreg[i];
  };

  // ---- MFMA role: wave w = output rows y = w * NRB + r, lane column jn = (r, x) ----------------------------------
  const int lr = jn / C::WB, lxo = jn % C::WB;
  f32x4 acc[C::TD];
  const u32x4* const wf = wq + lane;
  const int ly = wave * C::NRB + lr;                                   // this lane's output row inside the tile
  const bool live = jn < C::NRB * C::WB;                               // lanes 14, 15 of a 14-wide column block idle

  PHASE_DECL;
  Item cur = decode(walk.t);
  issue(cur, 0);
  PHASE_MARK(0);
#pragma unroll 1
  for (int t = walk.t; t < walk.end; t += walk.step) {
    const int tn = t + walk.step;
    const bool has_next = C::PERSIST && tn < walk.end;
    const Item nxt = decode(has_next ? tn : t);
#pragma unroll
    for (int z = 0; z < C::TD; ++z) acc[z] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int chunk = 0; chunk < C::NCH; ++chunk) {
      __syncthreads();                 // the previous chunk's MFMAs / the previous item's output staging are done with the LDS
      commit();
      if (chunk == 0 && tid < 16) xs[(tid >> 3) * C::NVOXP + C::NVOX + (tid & 7)] = (u32x4){0u, 0u, 0u, 0u};   // pad slots stay finite
      __syncthreads();
      PHASE_MARK(1);
      if (chunk + 1 < C::NCH) issue(cur, chunk + 1);
      else if (XPRE && has_next) issue(nxt, 0);
#ifndef V3D_CG_KYU
#define V3D_CG_KYU 1
#endif
#pragma unroll V3D_CG_KYU
      for (int ky = 0; ky < 3; ++ky) {
        bf16x8 a_hi[C::NKZ], a_lo[C::NKZ];
#pragma unroll
        for (int kz = 0; kz < C::NKZ; ++kz) {
          a_hi[kz] = __builtin_bit_cast(bf16x8, wf[((kz * 3 + ky) * 2) * 64]);
          a_lo[kz] = __builtin_bit_cast(bf16x8, wf[((kz * 3 + ky) * 2 + 1) * 64]);
        }
        const int rowbase = (C::S * (wave * C::NRB + lr) + ky) * C::IW + C::S * lxo + kq;
#pragma unroll
        for (int iz = 0; iz < C::ID; ++iz) {
          const bf16x8 b_hi = __builtin_bit_cast(bf16x8, xs[rowbase + iz * C::IH * C::IW]);
          const bf16x8 b_lo = __builtin_bit_cast(bf16x8, xs[rowbase + iz * C::IH * C::IW + C::NVOXP]);
#pragma unroll
          for (int kz = 0; kz < C::NKZ; ++kz) {
            const int z2 = iz - kz;
            if (z2 >= 0 && z2 % C::S == 0 && z2 / C::S < C::TD)
              acc[z2 / C::S] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[kz], b_hi, acc[z2 / C::S], 0, 0, 0);
          }
#pragma unroll
          for (int kz = 0; kz < C::NKZ; ++kz) {
            const int z2 = iz - kz;
            if (z2 >= 0 && z2 % C::S == 0 && z2 / C::S < C::TD)
              acc[z2 / C::S] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[kz], b_lo, acc[z2 / C::S], 0, 0, 0);
          }
#pragma unroll
          for (int kz = 0; kz < C::NKZ; ++kz) {
            const int z2 = iz - kz;
            if (z2 >= 0 && z2 % C::S == 0 && z2 / C::S < C::TD)
              acc[z2 / C::S] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo[kz], b_hi, acc[z2 / C::S], 0, 0, 0);
          }
        }
      }
      PHASE_MARK(2);
    }
    __syncthreads();                 // the input tile is dead: its LDS stages the output tile
    PHASE_MARK(3);

    // ---- bias + ReLU, through LDS, out in 16-byte (split layout) and / or 8-byte (fp32 rows) pieces ---------------
    const int cg = cur.cg, n = cur.n, oz0 = cur.oz0, oy0 = cur.oy0, ox0 = cur.ox0;
    float vout[C::TD][4];
    {
      // the bias comes through SGPRs (a per-lane vector load here would make the epilogue wait for the prefetched tile)
      float bias[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float b0 = bias_r[cg * 16 + r], b1 = bias_r[cg * 16 + 4 + r], b2 = bias_r[cg * 16 + 8 + r], b3 = bias_r[cg * 16 + 12 + r];
        bias[r] = lane_select(kq & 2, lane_select(kq & 1, b3, b2), lane_select(kq & 1, b1, b0));
      }
#pragma unroll
      for (int z = 0; z < C::TD; ++z)
#pragma unroll
        for (int r = 0; r < 4; ++r) vout[z][r] = fmaxf(acc[z][r] + bias[r], 0.f);
    }
    if constexpr ((C::OUT & kOutSplit) != 0) {
      u32x2* const sp2 = reinterpret_cast<u32x2*>(smem);               // [2 groups][hi, lo][NVO] slots, 8-byte halves
#pragma unroll
      for (int z = 0; z < C::TD; ++z) {
        if (!live) break;
        u32x2 hp, lp;
        split4(vout[z][0], vout[z][1], vout[z][2], vout[z][3], hp, lp);
        const int vox = (z * C::TH + ly) * C::TW + lxo;
        sp2[((((kq >> 1) * 2 + 0) * C::NVO) + vox) * 2 + (kq & 1)] = hp;
        sp2[((((kq >> 1) * 2 + 1) * C::NVO) + vox) * 2 + (kq & 1)] = lp;
      }
      __syncthreads();
      char* const outs = reinterpret_cast<char*>(reinterpret_cast<u32x4*>(p.out_split) + ((size_t)n * (C::COUT / 8) + cg * 2) * 2 * out_plane);
      const u32x4* const sq = reinterpret_cast<const u32x4*>(smem);
      for (int i = tid; i < 4 * C::NVO; i += 256) {
        const unsigned gp = v3d::small_div<C::NVO>((unsigned)i), vox = (unsigned)i - gp * C::NVO;
        const unsigned vz = v3d::small_div<C::TH * C::TW>(vox), vr = vox - vz * (C::TH * C::TW);
        const unsigned vy = v3d::small_div<C::TW>(vr), vx = vr - vy * C::TW;
        const int gz = oz0 + (int)vz, gy = oy0 + (int)vy, gx = ox0 + (int)vx;
        // (32-bit slot index on the wave-uniform base of the item's first plane, as in the staging loads)
        const unsigned idx = __umul24(gp, (unsigned)out_plane) + __umul24(__umul24(gz, p.Ho) + gy, p.Wo) + gx;
        if (gz < p.Do && gy < p.Ho && gx < p.Wo) *reinterpret_cast<u32x4*>(outs + idx * 16u) = sq[i];
      }
      if constexpr ((C::OUT & kOutF32) != 0) __syncthreads();
    }
    if constexpr ((C::OUT & kOutF32) != 0) {
      constexpr int OCS = C::NVO + 2;
      float* const os = reinterpret_cast<float*>(smem);                // [16 co][NVO (+2)]
      if (live) {
#pragma unroll
        for (int z = 0; z < C::TD; ++z)
#pragma unroll
          for (int r = 0; r < 4; ++r) os[(4 * kq + r) * OCS + (z * C::TH + ly) * C::TW + lxo] = vout[z][r];
      }
      __syncthreads();
      constexpr int NR = C::TD * C::TH, QPR = C::TW / 2;
      for (int i = tid; i < 16 * NR * QPR; i += 256) {
        const int co = i / (NR * QPR), row = (i / QPR) % NR, q = i % QPR;
        const int gz = oz0 + row / C::TH, gy = oy0 + row % C::TH, gx = ox0 + 2 * q;
        if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;
        const float2 v = *reinterpret_cast<const float2*>(os + co * OCS + row * C::TW + 2 * q);
        float* o = p.out_f32 + ((size_t)n * C::COUT + cg * 16 + co) * out_plane + ((size_t)gz * p.Ho + gy) * p.Wo + gx;
        if (gx + 1 < p.Wo && (p.Wo & 1) == 0) *reinterpret_cast<float2*>(o) = v;
        else { o[0] = v.x; if (gx + 1 < p.Wo) o[1] = v.y; }
      }
    }
    PHASE_MARK(4);
    if (!C::PERSIST) break;
    cur = nxt;
  }
  PHASE_FLUSH;
}

// ---- conv7 / conv8 (transposed convolutions + skip) on split-bf16 matrix cores -------------------------------------
// ConvTranspose3d(k 3, stride 2, pad 1, output_padding 1): per axis out[2j] = in[j] w[1], out[2j+1] = in[j] w[2] +
// in[j+1] w[0].  Cell j = outputs (2j, 2j+1) from inputs (j, j+1).  GEMM per chunk of 8 input channels: columns = the
// cells of an x row, rows = 16 output channels of one of the 8 output parities, K = 32 = (dy, dx) x 8 channels; the
// (pz, dz) combinations (0,0), (1,0), (1,1) x 4 (py, px) parities = 12 blocks of weights (zero where a parity does not
// see an input).  A wave keeps the B fragments of its two cell rows in registers and walks the 12 blocks.
// Input: split channel-last layout; output = ReLU(BN(deconv)) + skip (fp32 [n, COUT, D, H, W]) as fp32 or split.
// SKIP_SPLIT (the fused chain): the skip tensor comes in the split layout its producer (conv2 / conv4) hands to the next encoder
// layer anyway -- skip = hi + lo, the 16 mantissa bits every other operand of this mode has, as conv9+prob reads the conv0
// skip -- so that the encoder layer does not write a second, fp32 copy of its output (conv2: 154 of 463 MB per 64 cfg2 views).
template <int CIN_, int COUT_, int WB_, int OUT_, bool SKIP_SPLIT_ = false>
struct DG {
  static constexpr int CIN = CIN_, COUT = COUT_, WB = WB_, OUT = OUT_;
  static constexpr bool SKIP_SPLIT = SKIP_SPLIT_;
  static constexpr int NCH = CIN / 8, NCG = COUT / 16;
  static constexpr int NRB = 16 / WB;                         // cell rows per MFMA column block
  static constexpr int CZ = 2, CY = 4 * NRB, CX = WB;         // cells per tile; wave w = cell rows w*NRB .. of both cz
  static constexpr int VZ = CZ + 1, VY = CY + 1, VX = CX + 2; // input voxels (+1 idle column)
  static constexpr int NVOX = VZ * VY * VX, NVOXP = NVOX + 8;
  static constexpr int WQ = 12 * 2 * 64;                      // 16-byte words of one chunk's weight image
  static constexpr int NSLOT = 2 * NVOX;
  static constexpr int NIT = (NSLOT + 255) / 256, NWIT = (WQ + 255) / 256;
  static constexpr int LDS_BYTES = (2 * NVOXP + WQ) * 16;
  static_assert(CIN % 8 == 0 && COUT % 16 == 0 && (WB == 14 || WB == 8), "shape");
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

struct DeconvGParams {
  const void* in;      // split layout [n][CIN/8][hi, lo][Di][Hi][Wi]
  const void* wp;      // [NCG][NCH][12][hi, lo][64 lanes][4 words]
  const float* bias;   // [COUT]
  const float* skip;   // [n, COUT, 2Di, 2Hi, 2Wi] fp32 -- or, SKIP_SPLIT, the split layout [n][COUT/8][hi, lo][2Di][2Hi][2Wi]
  float* out_f32;      // same shape, or null
  void* out_split;     // split layout, or null
  int n, Di, Hi, Wi, ntz, nty, ntx;
  unsigned m_tx, m_ty, m_tz;   // v3d::magic_u32() of ntx, nty, ntz for the tile index (0: divide)
};

template <class C>
__global__ __launch_bounds__(256, 2) void deconvg_bf16x2_kernel(DeconvGParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS_BYTES];
  u32x4* const xs = reinterpret_cast<u32x4*>(smem);                 // [hi, lo][NVOXP]
  u32x4* const wq = xs + 2 * C::NVOXP;                              // [12][hi, lo][64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const int cg = blockIdx.y;
  const unsigned b0 = (unsigned)v3d::xcd_contiguous_block();
  const unsigned b1 = v3d::udiv_magic(b0, (unsigned)p.ntx, p.m_tx), b2 = v3d::udiv_magic(b1, (unsigned)p.nty, p.m_ty);
  const unsigned b3 = v3d::udiv_magic(b2, (unsigned)p.ntz, p.m_tz);
  const int tx = (int)(b0 - b1 * (unsigned)p.ntx), ty = (int)(b1 - b2 * (unsigned)p.nty), tz = (int)(b2 - b3 * (unsigned)p.ntz);
  const int n = (int)b3;
  const int cz0 = tz * C::CZ, cy0 = ty * C::CY, cx0 = tx * C::CX;   // first cell = first input voxel of the tile
  const int Do = 2 * p.Di, Ho = 2 * p.Hi, Wo = 2 * p.Wi;
  const size_t in_plane = (size_t)p.Di * p.Hi * p.Wi;
  const size_t out_plane = (size_t)Do * Ho * Wo;

  const u32x4* const ins = reinterpret_cast<const u32x4*>(p.in) + (size_t)n * C::NCH * 2 * in_plane;
  const u32x4* const wg = reinterpret_cast<const u32x4*>(p.wp) + (size_t)cg * C::NCH * C::WQ;
  u32x4 pre[C::NIT], wreg[C::NWIT];
  static_assert(C::NIT * 256 * C::NVOX < (1 << 20), "v3d::small_div range of the staging index");
  auto issue = [&](int chunk) __attribute__((always_inline)) {
    // (32-bit slot offsets on the chunk's wave-uniform base, as in convg_bf16x2_kernel; the host checks the range)
    const char* const insc = reinterpret_cast<const char*>(ins + (size_t)chunk * 2 * in_plane);
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const unsigned i = (unsigned)(it * 256 + tid);
      const unsigned part = v3d::small_div<C::NVOX>(i), v = i - part * C::NVOX;
      const unsigned vz = v3d::small_div<C::VY * C::VX>(v), vr = v - vz * (C::VY * C::VX);
      const unsigned vy = v3d::small_div<C::VX>(vr), vx = vr - vy * C::VX;
      const int gz = cz0 + (int)vz, gy = cy0 + (int)vy, gx = cx0 + (int)vx;
      const bool ok = i < C::NSLOT && gz < p.Di && gy < p.Hi && gx < p.Wi;       // inputs past the volume do not exist
      const int zc = min(gz, p.Di - 1), yc = min(gy, p.Hi - 1), xc = min(gx, p.Wi - 1);
      const unsigned idx = (part ? (unsigned)in_plane : 0u) + __umul24(__umul24(zc, p.Hi) + yc, p.Wi) + xc;
      const u32x4 val = *reinterpret_cast<const u32x4*>(insc + idx * 16u);
      pre[it] = ok ? val : (u32x4){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i)
      wreg[i] = (i * 256 + tid < C::WQ) ? wg[(size_t)chunk * C::WQ + i * 256 + tid] : (u32x4){0u, 0u, 0u, 0u};
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const unsigned i = (unsigned)(it * 256 + tid), part = v3d::small_div<C::NVOX>(i);
      if (i < C::NSLOT) xs[part * C::NVOXP + (i - part * C::NVOX)] = pre[it];
    }
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i)
      if (i * 256 + tid < C::WQ) wq[i * 256 + tid] = wreg[i];
  };
  if (tid < 16) xs[(tid >> 3) * C::NVOXP + C::NVOX + (tid & 7)] = (u32x4){0u, 0u, 0u, 0u};

  // column jn = (cell row r within the wave's pair, cell x); K lane group kq = (dy, dx)
  const int lr = jn / C::WB, lxo = jn % C::WB;
  const int lcy = wave * C::NRB + lr;
  f32x4 acc[C::CZ][8];
#pragma unroll
  for (int z = 0; z < C::CZ; ++z)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[z][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u32x4* const wf = wq + lane;

  issue(0);
#pragma unroll 1
  for (int chunk = 0; chunk < C::NCH; ++chunk) {
    __syncthreads();
    commit();
    __syncthreads();
    if (chunk + 1 < C::NCH) issue(chunk + 1);
    // B fragments of this wave's cell rows: input planes cz .. cz + 1 for cz = 0 .. CZ-1 => VZ planes
    bf16x8 b_hi[C::VZ], b_lo[C::VZ];
#pragma unroll
    for (int vz = 0; vz < C::VZ; ++vz) {
      const int slot = (vz * C::VY + lcy + (kq >> 1)) * C::VX + lxo + (kq & 1);
      b_hi[vz] = __builtin_bit_cast(bf16x8, xs[slot]);
      b_lo[vz] = __builtin_bit_cast(bf16x8, xs[slot + C::NVOXP]);
    }
#pragma unroll
    for (int pyx = 0; pyx < 4; ++pyx) {
#pragma unroll
      for (int zb = 0; zb < 3; ++zb) {                        // (pz, dz) = (0,0), (1,0), (1,1)
        const int pz = zb == 0 ? 0 : 1, dz = zb == 2 ? 1 : 0;
        const bf16x8 a_hi = __builtin_bit_cast(bf16x8, wf[((zb * 4 + pyx) * 2) * 64]);
        const bf16x8 a_lo = __builtin_bit_cast(bf16x8, wf[((zb * 4 + pyx) * 2 + 1) * 64]);
#pragma unroll
        for (int cz = 0; cz < C::CZ; ++cz) {
          f32x4& c = acc[cz][pz * 4 + pyx];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi[cz + dz], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo[cz + dz], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi[cz + dz], c, 0, 0, 0);
        }
      }
    }
  }

  // ---- BN bias + ReLU + skip; the two x parities of a cell are one float2 / adjacent slots ----------------------------
  const bool live = jn < C::NRB * C::WB;
  const int gcy = cy0 + lcy, gcx = cx0 + lxo;
  if (live && gcy < p.Hi && gcx < p.Wi) {
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = p.bias[cg * 16 + 4 * kq + r];
#pragma unroll
    for (int cz = 0; cz < C::CZ; ++cz) {
      const int gcz = cz0 + cz;
      if (gcz >= p.Di) break;
#pragma unroll
      for (int pzy = 0; pzy < 4; ++pzy) {
        const int pz = pzy >> 1, py = pzy & 1;
        const size_t sp = ((size_t)(2 * gcz + pz) * Ho + (2 * gcy + py)) * Wo + 2 * gcx;
        float v0[4], v1[4];
        float sk0[4], sk1[4];
        if constexpr (C::SKIP_SPLIT) {
          // channels 4 kq .. 4 kq + 3 of group cg * 2 + (kq >> 1): one 8-byte half of the hi / lo slots of the two voxels
          const u32x2* const ss = reinterpret_cast<const u32x2*>(p.skip) +
                                  (((size_t)n * (C::COUT / 8) + cg * 2 + (kq >> 1)) * 2 * out_plane) * 2 + (kq & 1);
          const u32x2 h0 = ss[sp * 2], h1 = ss[(sp + 1) * 2], l0 = ss[(out_plane + sp) * 2], l1 = ss[(out_plane + sp + 1) * 2];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned sh = (r & 1) ? 0u : 16u, mk = (r & 1) ? 0xffff0000u : 0xffffffffu;
            sk0[r] = __uint_as_float((h0[r >> 1] << sh) & mk) + __uint_as_float((l0[r >> 1] << sh) & mk);
            sk1[r] = __uint_as_float((h1[r >> 1] << sh) & mk) + __uint_as_float((l1[r >> 1] << sh) & mk);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t o = ((size_t)n * C::COUT + cg * 16 + 4 * kq + r) * out_plane + sp;
          if constexpr (!C::SKIP_SPLIT) {
            const float2 sk = *reinterpret_cast<const float2*>(p.skip + o);
            sk0[r] = sk.x; sk1[r] = sk.y;
          }
          v0[r] = fmaxf(acc[cz][pz * 4 + py * 2 + 0][r] + bias[r], 0.f) + sk0[r];
          v1[r] = fmaxf(acc[cz][pz * 4 + py * 2 + 1][r] + bias[r], 0.f) + sk1[r];
          if constexpr ((C::OUT & kOutF32) != 0) *reinterpret_cast<float2*>(p.out_f32 + o) = make_float2(v0[r], v1[r]);
        }
        if constexpr ((C::OUT & kOutSplit) != 0) {
          // this lane holds channels 4 kq .. 4 kq + 3 of group cg * 2 + (kq >> 1): one 8-byte half of the hi / lo slot
          u32x2* const os = reinterpret_cast<u32x2*>(p.out_split) +
                            (((size_t)n * (C::COUT / 8) + cg * 2 + (kq >> 1)) * 2 * out_plane) * 2 + (kq & 1);
          u32x2 h0, l0, h1, l1;
          split4(v0[0], v0[1], v0[2], v0[3], h0, l0);
          split4(v1[0], v1[1], v1[2], v1[3], h1, l1);
          os[sp * 2] = h0;
          os[(sp + 1) * 2] = h1;
          os[(out_plane + sp) * 2] = l0;
          os[(out_plane + sp + 1) * 2] = l1;
        }
      }
    }
  }
}

// ---- fp32 [n, C, D, H, W] -> split channel-last layout (per-layer entry point of the split kernels) ----------------
__global__ __launch_bounds__(256) void encode_split_kernel(const float* __restrict__ in, u32x4* __restrict__ out, int C,
                                                           size_t plane, size_t total) {   // total = n * (C / 8) * plane
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t sp = i % plane, ng = i / plane;                 // ng = n * (C / 8) + group
  const float* src = in + (ng * 8) * plane + sp;               // channels of a group are consecutive planes
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = src[(size_t)c * plane];
  u32x2 ha, la, hb, lb;
  split4(v[0], v[1], v[2], v[3], ha, la);
  split4(v[4], v[5], v[6], v[7], hb, lb);
  out[(ng * 2) * plane + sp] = (u32x4){ha.x, ha.y, hb.x, hb.y};
  out[(ng * 2 + 1) * plane + sp] = (u32x4){la.x, la.y, lb.x, lb.y};
}

template <class C>
int launch_convg(const char* name, const void* in, const float* wbf, const float* bias, float* out_f32, void* out_split,
                 int n, int Di, int Hi, int Wi, hipStream_t s) {
  ConvGParams p;
  p.in = in; p.wp = wbf; p.bias = bias; p.out_f32 = out_f32; p.out_split = out_split; p.n = n;
  p.Di = Di; p.Hi = Hi; p.Wi = Wi;
  p.Do = (Di - 1) / C::S + 1; p.Ho = (Hi - 1) / C::S + 1; p.Wo = (Wi - 1) / C::S + 1;
  V3D_REQUIRE(((C::OUT & kOutF32) == 0 || out_f32) && ((C::OUT & kOutSplit) == 0 || out_split), V3D_ERR_BAD_ARG,
              "%s: missing output buffer", name);
  // 32-bit slot offsets inside one (view, channel group): 2 (hi, lo) x plane x 16 bytes < 4 GB; the output side indexes 4 planes
  // from the item's base
  TileGrid g;
  if (const int rc = tile_grid(name, n, p.Do, p.Ho, p.Wo, C::TD, C::TH, C::TW, 0, Di, Hi, Wi, 1ll << 24, &g); rc != V3D_OK) return rc;
  p.ntz = g.ntz; p.nty = g.nty; p.ntx = g.ntx; p.m_tx = g.m_tx; p.m_ty = g.m_t1; p.m_tz = g.m_t2;
  const long long blocks = g.blocks;
  static bool lds_opted[64] = {};
  if (const int rc = v3d::opt_in_dynamic_lds((const void*)convg_bf16x2_kernel<C>, (int)C::LDS_BYTES, lds_opted); rc != V3D_OK) return rc;
  {
    v3d::TimedScope ts(name, s);
    unsigned grid = (unsigned)((blocks * C::NCG + 7) / 8 * 8);        // one (tile, channel group) item per workgroup ...
    if (C::PERSIST) {                                                  // ... or as many workgroups as the chip holds
      static int wgs_per_cu = 0;
      if (wgs_per_cu == 0) {
        int nb = 0;
        V3D_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)convg_bf16x2_kernel<C>, 256, C::LDS_BYTES));
        wgs_per_cu = nb > 0 ? nb : 1;
      }
      grid = v3d::persistent_grid(blocks * C::NCG, wgs_per_cu);
    }
    convg_bf16x2_kernel<C><<<grid, 256, C::LDS_BYTES, s>>>(p, p.bias);
  }
  V3D_CHECK_LAUNCH(name);
  return V3D_OK;
}

template <class C>
int launch_deconvg(const char* name, const void* in, const float* wbf, const float* bias, const float* skip, float* out_f32,
                   void* out_split, int n, int Di, int Hi, int Wi, hipStream_t s) {
  DeconvGParams p;
  p.in = in; p.wp = wbf; p.bias = bias; p.skip = skip; p.out_f32 = out_f32; p.out_split = out_split; p.n = n;
  p.Di = Di; p.Hi = Hi; p.Wi = Wi;
  V3D_REQUIRE(skip && ((C::OUT & kOutF32) == 0 || out_f32) && ((C::OUT & kOutSplit) == 0 || out_split), V3D_ERR_BAD_ARG,
              "%s: missing buffer", name);
  TileGrid g;
  if (const int rc = tile_grid(name, n, Di, Hi, Wi, C::CZ, C::CY, C::CX, 0, Di, Hi, Wi, 1ll << 24, &g); rc != V3D_OK) return rc;
  p.ntz = g.ntz; p.nty = g.nty; p.ntx = g.ntx; p.m_tx = g.m_tx; p.m_ty = g.m_t1; p.m_tz = g.m_t2;
  {
    v3d::TimedScope ts(name, s);
    deconvg_bf16x2_kernel<C><<<dim3((unsigned)g.blocks, C::NCG), 256, 0, s>>>(p);
  }
  V3D_CHECK_LAUNCH(name);
  return V3D_OK;
}

// The kernel configuration of every layer, stated once: CG<Cin, Cout, stride, row width of the MFMA column block, outputs>,
// DG<Cin, Cout, row width, outputs, skip in the split layout>
template <int OUT> using Conv1 = CG<8, 16, 2, 14, OUT>;
template <int OUT> using Conv2 = CG<16, 16, 1, 14, OUT>;
template <int OUT> using Conv3 = CG<16, 32, 2, 14, OUT>;
template <int OUT> using Conv4 = CG<32, 32, 1, 14, OUT>;
template <int OUT> using Conv5 = CG<32, 64, 2, 8, OUT>;
template <int OUT> using Conv6 = CG<64, 64, 1, 8, OUT>;
template <int OUT> using Conv7 = DG<64, 32, 8, OUT, OUT == kOutSplit>;
template <int OUT> using Conv8 = DG<32, 16, 14, OUT, OUT == kOutSplit>;

template <int OUT>
int launch_layer(int layer, const void* in, const float* wbf, const float* bias, const float* skip, float* out_f32, void* out_split,
                 int n, int Di, int Hi, int Wi, hipStream_t s) {
  switch (layer) {
    case 1: return launch_convg<Conv1<OUT>>("costreg_conv1", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 2: return launch_convg<Conv2<OUT>>("costreg_conv2", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 3: return launch_convg<Conv3<OUT>>("costreg_conv3", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 4: return launch_convg<Conv4<OUT>>("costreg_conv4", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 5: return launch_convg<Conv5<OUT>>("costreg_conv5", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 6: return launch_convg<Conv6<OUT>>("costreg_conv6", in, wbf, bias, out_f32, out_split, n, Di, Hi, Wi, s);
    case 7: return launch_deconvg<Conv7<OUT>>("costreg_conv7", in, wbf, bias, skip, out_f32, out_split, n, Di, Hi, Wi, s);
    case 8: return launch_deconvg<Conv8<OUT>>("costreg_conv8", in, wbf, bias, skip, out_f32, out_split, n, Di, Hi, Wi, s);
  }
  return fail(V3D_ERR_BAD_ARG, "costreg: layer %d is not one of conv1..conv8", layer);
}

}  // namespace

int launch_split_layer(int layer, int out, const void* in, const float* wbf, const float* bias, const void* skip, void* dst, int n,
                       int Di, int Hi, int Wi, hipStream_t s) {
  if (out == kOutF32) return launch_layer<kOutF32>(layer, in, wbf, bias, (const float*)skip, (float*)dst, nullptr, n, Di, Hi, Wi, s);
  return launch_layer<kOutSplit>(layer, in, wbf, bias, (const float*)skip, nullptr, dst, n, Di, Hi, Wi, s);
}

int launch_encode_split(const float* in, void* out, int C, size_t plane, size_t total, hipStream_t s) {
  encode_split_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(in, (u32x4*)out, C, plane, total);
  V3D_CHECK_LAUNCH("encode_split_kernel");
  return V3D_OK;
}

// split-bf16 image of conv1..conv6 for convg_bf16x2_kernel: [cout group][8-channel chunk][kz, ky][hi, lo][lane 64]
// [4 words]; rows = output channel within the group, k = 8 * x tap + ci (x tap 3 = 0)
void pack_convg(const float* w, int cin, int cout, unsigned* wb) {
  const int nch = cin / 8, ncg = cout / 16;
  for (int g = 0; g < ncg; ++g)
    for (int ch = 0; ch < nch; ++ch)
      for (int kzy = 0; kzy < 9; ++kzy)
        for (int lane = 0; lane < 64; ++lane) {
          const int co = g * 16 + (lane & 15), kx = lane >> 4;
          float v[8];
          for (int e = 0; e < 8; ++e) v[e] = kx > 2 ? 0.f : w[((size_t)co * cin + ch * 8 + e) * 27 + kzy * 3 + kx];
          unsigned* dst = wb + (((size_t)g * nch + ch) * 9 + kzy) * 2 * kLoWords + lane * 4;
          v3d::split_bf16x8(v, dst, dst + kLoWords);
        }
}

// split-bf16 image of conv7 / conv8 for deconvg_bf16x2_kernel, w = ConvTranspose3d weight [cin][cout][27]: [cout group]
// [8-channel chunk][block 12][hi, lo][lane 64][4 words]; block = zb * 4 + (py, px), zb = {(pz 0, dz 0), (1, 0), (1, 1)};
// rows = output channel, k = 8 * (dy, dx) + ci.  Kernel tap of (parity p, input d): p 0: d 0 -> 1; p 1: d 0 -> 2, d 1 -> 0.
void pack_deconvg(const float* w, int cin, int cout, unsigned* wb) {
  const int nch = cin / 8, ncg = cout / 16;
  auto tap = [](int par, int d) { return par == 0 ? (d == 0 ? 1 : -1) : (d == 0 ? 2 : 0); };
  for (int g = 0; g < ncg; ++g)
    for (int ch = 0; ch < nch; ++ch)
      for (int blk = 0; blk < 12; ++blk)
        for (int lane = 0; lane < 64; ++lane) {
          const int zb = blk / 4, py = (blk >> 1) & 1, px = blk & 1;
          const int pz = zb == 0 ? 0 : 1, dz = zb == 2 ? 1 : 0;
          const int co = g * 16 + (lane & 15), dy = lane >> 5, dx = (lane >> 4) & 1;
          const int kz = tap(pz, dz), ky = tap(py, dy), kx = tap(px, dx);
          float v[8];
          for (int e = 0; e < 8; ++e)
            v[e] = (kz < 0 || ky < 0 || kx < 0) ? 0.f : w[((size_t)(ch * 8 + e) * cout + co) * 27 + kz * 9 + ky * 3 + kx];
          unsigned* dst = wb + (((size_t)g * nch + ch) * 12 + blk) * 2 * kLoWords + lane * 4;
          v3d::split_bf16x8(v, dst, dst + kLoWords);
        }
}

}  // namespace v3d
