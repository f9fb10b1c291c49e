// CostRegNet, the exact-fp32 per-layer kernels (v3d_costreg_layer_f32, and conv0..conv8 of the chain with precision =
// V3D_PRECISION_FP32; costreg.hip is the map of the family): one templated implicit-GEMM kernel on v_mfma_f32_16x16x4_f32
// (bitwise an fmaf chain).  They were the first correct path and remain the reference point for the split kernels' per-layer
// parity tests.
//
//   D[co, voxel] += W'[co, k] * X[k, voxel],  k = (input channel, kernel tap)
//
//   * A operand = BN-folded weights, pre-packed on the host into MFMA fragment order (one coalesced
//     256-B global load per fragment, L2-resident, shared by every workgroup);
//   * B operand = activations: a halo'd input tile of CK channels is staged in LDS channel-major
//     ([ck][z][y][x], plane stride chosen so the 4 k-lanes x 16 voxel-lanes of a ds_read_b32 hit
//     distinct banks); zero padding is materialised in the tile so the inner loop has no bounds
//     checks; every output voxel of the tile owns a per-lane LDS base offset, every kernel tap is a
//     wave-uniform offset on top of it;
//   * each wave keeps NBW voxel blocks x MB channel blocks of 16x16 accumulators in registers
//     across all input-channel chunks; epilogue = +bias, ReLU, optional skip add (after the ReLU,
//     mvsnet.py:159-161), store in the reference's [n, C, D, H, W] layout (16 consecutive voxels
//     per store row);
//   * stride-2 conv reads the tile with stride 2; the stride-2 transposed conv (k3, p1,
//     output_padding 1) is decomposed into its 8 output-parity classes, each a dense gather with
//     1..8 taps (out[o] = sum_k in[(o+1-k)/2] W[k] for (o+1-k) even).
#include "costreg.h"
#include "phase_timing.h"

#ifndef V3D_ABLATE
#define V3D_ABLATE 0   // developer ablations of the conv kernel (1: no MFMA loop, 2: no restaging)
#endif

PHASE_TIMING_UNIT(v3d_debug_fp32_phase_read)

namespace v3d {
namespace {

// kConvS1 / kConvS2: k3 p1 conv with stride 1 / 2.  kDeconvS2: k3 s2 p1 output_padding-1 transposed
// conv.  kConvS1Pair: stride-1 conv for COUT == 8 -- the 16 MFMA rows hold 2 x-shifts x 8 output
// channels over a 4-wide x window (36 "virtual taps", the weight image is zero where the shifted
// kernel does not reach), each voxel block is 16 x-PAIRS: 18 MFMAs per 16 output voxels instead of
// the 27 a half-empty 16-row tile would cost.
enum { kConvS1 = 0, kConvS2 = 1, kDeconvS2 = 2, kConvS1Pair = 3 };

template <int MODE_, int CIN_, int COUT_, int TD_, int TH_, int TW_, int CK_, int OCC_ = 2>
struct ConvCfg {
  static constexpr int OCC = OCC_;   // min waves per SIMD (register budget 512 / OCC)
  static constexpr int MODE = MODE_, CIN = CIN_, COUT = COUT_, TD = TD_, TH = TH_, TW = TW_, CK = CK_;
  static constexpr bool S1LIKE = MODE == kConvS1 || MODE == kConvS1Pair;
  static constexpr int MB = MODE == kConvS1Pair ? 1 : (COUT + 15) / 16;
  static constexpr int ID = S1LIKE ? TD + 2 : MODE == kConvS2 ? 2 * TD + 1 : TD / 2 + 1;
  static constexpr int IH = S1LIKE ? TH + 2 : MODE == kConvS2 ? 2 * TH + 1 : TH / 2 + 1;
  static constexpr int IW = S1LIKE ? TW + 2 : MODE == kConvS2 ? 2 * TW + 1 : TW / 2 + 1;
  static constexpr int PLANE = ID * IH * IW;
  // channel-plane stride in LDS: odd where lanes read with x stride 2, == 16 (mod 32) otherwise
  static constexpr int S = (MODE == kConvS2 || MODE == kConvS1Pair)
                               ? (PLANE | 1) : ((PLANE - 16 + 31) / 32) * 32 + 16;
  static constexpr int KXN = MODE == kConvS1Pair ? 4 : 3;   // x taps
  static constexpr int NT = 9 * KXN;                        // (virtual) taps per input channel
  static constexpr int NVOX = TD * TH * TW;
  static constexpr int NCLS = MODE == kDeconvS2 ? 8 : 1;
  // lattice the voxel blocks enumerate: parity sub-lattice (deconv), x pairs (pair mode)
  static constexpr int CD = MODE == kDeconvS2 ? TD / 2 : TD;
  static constexpr int CH = MODE == kDeconvS2 ? TH / 2 : TH;
  static constexpr int CW = (MODE == kDeconvS2 || MODE == kConvS1Pair) ? TW / 2 : TW;
  static constexpr int NVC = CD * CH * CW;
  static constexpr int NBC = (NVC + 15) / 16;
  static constexpr int NBT = NBC * NCLS;
  static constexpr int NBW = (NBT + 3) / 4;
  static constexpr int NCHUNK = CIN / CK;
  static constexpr int C4 = CK / 4;
  static constexpr int LDS_BYTES = CK * S * 4;
  // staging geometry
  static constexpr int IWP = IW <= 8 ? 8 : IW <= 16 ? 16 : IW <= 32 ? 32 : 64;
  static constexpr int RPW = 64 / IWP;                     // rows per wave per iteration
  static constexpr int ROWS = CK * ID * IH;
  static constexpr int NIT = (ROWS + 4 * RPW - 1) / (4 * RPW);
  static constexpr int SU = NIT < 10 ? NIT : 10;           // rows in flight per lane
  // Prefetch mode: the next channel chunk's tile rows AND its weight fragments are loaded into
  // registers right after the barrier and stay in flight during the whole MFMA loop; A fragments are
  // then served from LDS (lgkmcnt) so that no vmcnt wait inside the loop drains the prefetch.
  static constexpr int WCH = NT * C4 * MB * 64;            // packed weight floats per chunk
  static constexpr int NWIT = (WCH + 255) / 256;
  static constexpr bool PF = WCH <= 8192 && (NIT + NWIT) <= 64 && (NIT + NWIT + 4 * NBW * MB) <= 150;
  static constexpr int TROWS = NIT * 4 * RPW;              // staging row-table entries (>= ROWS)
  static constexpr int LDS_FLOATS = CK * S + (PF ? WCH : 0) + 2 * TROWS;
  static_assert(IW <= 64, "tile row wider than a wave");
  static_assert(CIN % CK == 0 && CK % 4 == 0, "channel chunking");
  static_assert(MODE != kDeconvS2 || (TD % 2 == 0 && TH % 2 == 0 && TW % 2 == 0), "even tile");
  static_assert(MODE != kDeconvS2 || NBW == 2 * NBC, "two parity classes per wave");
  static_assert(MODE != kConvS1Pair || (COUT == 8 && TW % 2 == 0), "pair mode: 8 channels, even TW");
  static_assert(LDS_FLOATS * 4 <= 64 * 1024, "LDS tile");
};

// VEC (stride-1 layers in prefetch mode, tile and volume widths multiples of 4): the halo'd rows are fetched as aligned float4s
// (16 lanes per row, [ix0 - 3, ix0 + 61)) instead of one float per lane -- the CU's vector-memory path charges a 4-byte-per-lane
// wave instruction twice the cycles of a 16-byte one for a quarter of the bytes.
template <class C, bool VEC>
__global__ __launch_bounds__(256, C::OCC) void conv3d_mfma_kernel(ConvParams p) {
  constexpr int MODE = C::MODE;
  __shared__ float xs[C::LDS_FLOATS];
  float* const ws = xs + C::CK * C::S;   // weight fragments of the current chunk (PF mode)
  // per-row staging tables, built once: global element offset of the row start (kRowOob if the
  // row lies outside the volume in z/y) and LDS element offset of the row (-1 = no such row)
  int* const rowg = reinterpret_cast<int*>(xs + C::CK * C::S + (C::PF ? C::WCH : 0));
  int* const rowd = rowg + C::TROWS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;

  int b = v3d::xcd_contiguous_block();     // neighbouring tiles (shared halo) on the same XCD's L2
  const int tx = b % p.ntx; b /= p.ntx;
  const int ty = b % p.nty; b /= p.nty;
  const int tz = b % p.ntz;
  const int n = b / p.ntz;
  const int oz0 = tz * C::TD, oy0 = ty * C::TH, ox0 = tx * C::TW;
  const int iz0 = C::S1LIKE ? oz0 - 1 : MODE == kConvS2 ? 2 * oz0 - 1 : oz0 / 2;
  const int iy0 = C::S1LIKE ? oy0 - 1 : MODE == kConvS2 ? 2 * oy0 - 1 : oy0 / 2;
  const int ix0 = C::S1LIKE ? ox0 - 1 : MODE == kConvS2 ? 2 * ox0 - 1 : ox0 / 2;

  // per-lane LDS base offset of each of this wave's voxel blocks
  int boff[C::NBW];
#pragma unroll
  for (int j = 0; j < C::NBW; ++j) {
    int i = MODE == kDeconvS2 ? (j % C::NBC) : (wave * C::NBW + j);
    int v = min(i * 16 + jn, C::NVC - 1);
    int z = v / (C::CH * C::CW), y = (v / C::CW) % C::CH, x = v % C::CW;
    int off = MODE == kConvS2 ? ((2 * z) * C::IH + 2 * y) * C::IW + 2 * x
            : MODE == kConvS1Pair ? (z * C::IH + y) * C::IW + 2 * x
                                  : (z * C::IH + y) * C::IW + x;
    boff[j] = off + kq * C::S;
  }

  f32x4 acc[C::NBW][C::MB];
#pragma unroll
  for (int j = 0; j < C::NBW; ++j)
#pragma unroll
    for (int m = 0; m < C::MB; ++m) acc[j][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const size_t in_plane = (size_t)p.Di * p.Hi * p.Wi;
  const float* inb = p.in + (size_t)n * C::CIN * in_plane;
  const float* wl = p.wp + lane;

  // A fragments (weights) are software-pipelined one tap ahead: fragment index f = chunk*NT + tap
  // walks the packed image linearly, so "next tap" also crosses chunk boundaries.
  constexpr int kLastFrag = C::NCHUNK * C::NT - 1;
  float a_cur[C::C4][C::MB], a_nxt[C::C4][C::MB];
  auto load_a = [&](float (&a)[C::C4][C::MB], int f) {
#pragma unroll
    for (int c4 = 0; c4 < C::C4; ++c4)
#pragma unroll
      for (int m = 0; m < C::MB; ++m) a[c4][m] = wl[((size_t)(f * C::C4 + c4) * C::MB + m) * 64];
  };
  if constexpr (MODE != kDeconvS2 && !C::PF) load_a(a_cur, 0);

  // staging lane role: a group of IWP lanes (IWP = IW rounded up to a power of two) copies one
  // (channel, z, y) row of the halo'd tile
  const int lrow = lane / C::IWP, lx = lane % C::IWP;
  const int sgx = ix0 + lx;
  const bool xok = lx < C::IW;
  const bool xin = xok && sgx >= 0 && sgx < p.Wi;
  constexpr int kRowOob = -2147483647 - 1;
  for (int r = tid; r < C::TROWS; r += 256) {
    const int ck = r / (C::ID * C::IH), rz = (r / C::IH) % C::ID, ry = r % C::IH;
    const int gz = iz0 + rz, gy = iy0 + ry;
    const bool in_vol = gz >= 0 && gz < p.Di && gy >= 0 && gy < p.Hi;
    rowg[r] = (r < C::ROWS && in_vol) ? ck * (int)in_plane + (gz * p.Hi + gy) * p.Wi + ix0 : kRowOob;
    rowd[r] = r < C::ROWS ? ck * C::S + (rz * C::IH + ry) * C::IW : -1;
  }
  __syncthreads();
  const int myrow0 = wave * C::RPW + lrow;        // this lane's rows: myrow0 + it * 4 * RPW

  constexpr int NITV = (C::ROWS + 15) / 16;     // VEC: 16 rows per workgroup iteration
  const int vj = tid & 15, vrow = tid >> 4;
  const int vgx = ix0 - 3 + 4 * vj;
  const bool vin = vgx >= 0 && vgx + 3 < p.Wi && 4 * vj - 3 < C::IW;
  float pre[(C::PF && !VEC) ? C::NIT : 1], wreg[C::PF ? C::NWIT : 1];
  f32x4 pre4[(C::PF && VEC) ? NITV : 1];
  auto pf_issue = [&](int chunk) {
    if constexpr (VEC) {
      const float* incv = inb + (size_t)chunk * C::CK * in_plane + (4 * vj - 3);
#pragma unroll
      for (int it = 0; it < NITV; ++it) {
        const int r = it * 16 + vrow;
        const int g = rowg[min(r, C::TROWS - 1)];
        pre4[it] = (r < C::ROWS && g != kRowOob && vin) ? *reinterpret_cast<const f32x4*>(incv + g) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    } else {
      const float* inc = inb + (size_t)chunk * C::CK * in_plane + lx;
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        const int g = rowg[myrow0 + it * 4 * C::RPW];
        pre[it] = (g != kRowOob && xin) ? inc[g] : 0.f;
      }
    }
    const float* wc = p.wp + (size_t)chunk * C::WCH + tid;
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i) wreg[i] = (i * 256 + tid < C::WCH) ? wc[i * 256] : 0.f;
  };
  auto pf_commit = [&]() {
    if constexpr (VEC) {
#pragma unroll
      for (int it = 0; it < NITV; ++it) {
        const int r = it * 16 + vrow;
        const int d = rowd[min(r, C::TROWS - 1)];
        if (r < C::ROWS && d >= 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = 4 * vj - 3 + e;
            if (x >= 0 && x < C::IW) xs[d + x] = pre4[it][e];
          }
        }
      }
    } else {
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        const int d = rowd[myrow0 + it * 4 * C::RPW];
        if (d >= 0 && xok) xs[d + lx] = pre[it];
      }
    }
#pragma unroll
    for (int i = 0; i < C::NWIT; ++i)
      if (i * 256 + tid < C::WCH) ws[i * 256 + tid] = wreg[i];
  };
  PHASE_DECL;
  if constexpr (C::PF) pf_issue(0);
  PHASE_MARK(0);

#pragma unroll 1
  for (int chunk = 0; chunk < C::NCHUNK; ++chunk) {
    __syncthreads();
    PHASE_MARK(1);
    if constexpr (C::PF) {
#if V3D_ABLATE == 2
      if (chunk == 0) pf_commit();
      __syncthreads();
#else
      pf_commit();
      PHASE_MARK(2);
      __syncthreads();
      PHASE_MARK(3);
      if (chunk + 1 < C::NCHUNK) pf_issue(chunk + 1);
      PHASE_MARK(4);
#endif
    } else {
      // batched staging: SU independent rows are in flight per lane before the LDS writes, so
      // global latency is paid once per batch rather than once per element
      const float* inc = inb + (size_t)chunk * C::CK * in_plane + lx;
#pragma unroll 1
      for (int it0 = 0; it0 < C::NIT; it0 += C::SU) {
        float v[C::SU];
#pragma unroll
        for (int u = 0; u < C::SU; ++u) {
          v[u] = 0.f;
          if (it0 + u < C::NIT) {
            const int g = rowg[myrow0 + (it0 + u) * 4 * C::RPW];
            if (g != kRowOob && xin) v[u] = inc[g];
          }
        }
#pragma unroll
        for (int u = 0; u < C::SU; ++u) {
          if (it0 + u < C::NIT) {
            const int d = rowd[myrow0 + (it0 + u) * 4 * C::RPW];
            if (d >= 0 && xok) xs[d + lx] = v[u];
          }
        }
      }
      __syncthreads();
    }

#if V3D_ABLATE == 1
    if (p.relu == 12345)
#endif
    if constexpr (MODE != kDeconvS2) {
#pragma unroll 1
      for (int kzy = 0; kzy < 9; ++kzy) {
        const int kz = kzy / 3, ky = kzy % 3;
#pragma unroll
        for (int kx = 0; kx < C::KXN; ++kx) {
          const int tap = kzy * C::KXN + kx;
          const int tapoff = (kz * C::IH + ky) * C::IW + kx;
          if constexpr (C::PF) {
#pragma unroll
            for (int c4 = 0; c4 < C::C4; ++c4)
#pragma unroll
              for (int m = 0; m < C::MB; ++m)
                a_cur[c4][m] = ws[((tap * C::C4 + c4) * C::MB + m) * 64 + lane];
          } else {
            load_a(a_nxt, min(chunk * C::NT + tap + 1, kLastFrag));
          }
#pragma unroll
          for (int c4 = 0; c4 < C::C4; ++c4) {
#pragma unroll
            for (int j = 0; j < C::NBW; ++j) {
              const float bv = xs[boff[j] + tapoff + c4 * 4 * C::S];
#pragma unroll
              for (int m = 0; m < C::MB; ++m)
                acc[j][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[c4][m], bv, acc[j][m], 0, 0, 0);
            }
          }
          if constexpr (!C::PF) {
#pragma unroll
            for (int c4 = 0; c4 < C::C4; ++c4)
#pragma unroll
              for (int m = 0; m < C::MB; ++m) a_cur[c4][m] = a_nxt[c4][m];
          }
        }
      }
    } else {
#pragma unroll
      for (int cl = 0; cl < 2; ++cl) {
        const int cls = wave * 2 + cl;
        const int pz = (cls >> 2) & 1, py = (cls >> 1) & 1, px = cls & 1;
#pragma unroll 1
        for (int tap = 0; tap < 27; ++tap) {
          const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
          // parity p == 0 (even output): only k = 1; p == 1: k = 0 (input c+1) and k = 2 (input c)
          if ((pz == 0) != (kz == 1)) continue;
          if ((py == 0) != (ky == 1)) continue;
          if ((px == 0) != (kx == 1)) continue;
          const int dz = kz == 0 ? 1 : 0, dy = ky == 0 ? 1 : 0, dx = kx == 0 ? 1 : 0;
          const int tapoff = (dz * C::IH + dy) * C::IW + dx;
          if constexpr (C::PF) {
#pragma unroll
            for (int c4 = 0; c4 < C::C4; ++c4)
#pragma unroll
              for (int m = 0; m < C::MB; ++m)
                a_cur[c4][m] = ws[((tap * C::C4 + c4) * C::MB + m) * 64 + lane];
          } else {
            load_a(a_cur, chunk * 27 + tap);
          }
#pragma unroll
          for (int c4 = 0; c4 < C::C4; ++c4) {
#pragma unroll
            for (int i = 0; i < C::NBC; ++i) {
              const float bv = xs[boff[cl * C::NBC + i] + tapoff + c4 * 4 * C::S];
#pragma unroll
              for (int m = 0; m < C::MB; ++m)
                acc[cl * C::NBC + i][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    a_cur[c4][m], bv, acc[cl * C::NBC + i][m], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  PHASE_MARK(5);
  // ---- epilogue: bias, ReLU, skip, store ([n, COUT, Do, Ho, Wo]) -------------------------------
  const size_t out_plane = (size_t)p.Do * p.Ho * p.Wo;
  // Where the whole output tile fits the (dead) input tile's LDS and rows are 16-byte addressable, it leaves through LDS as
  // float4 row segments with float4 skip loads.  The direct paths below issue 4- or 8-byte skip loads and stores per (channel,
  // voxel) and lane: on conv9 (8 channels at full resolution) that epilogue was 75 % of the workgroup's time.
  constexpr int OCS = C::NVOX + 4;                 // channel stride of the staged tile (padded against bank conflicts)
  constexpr bool kStage = C::COUT * OCS <= C::LDS_FLOATS && C::TW % 4 == 0;
  const bool staged = kStage && (p.Wo & 3) == 0 &&
                      ((reinterpret_cast<size_t>(p.out) | reinterpret_cast<size_t>(p.skip)) & 15) == 0;
  float* const os = xs;
  auto stage_value = [&](int co, int z, int y, int x, float val) __attribute__((always_inline)) {
    val += p.bias[co];
    if (p.relu) val = fmaxf(val, 0.f);
    os[co * OCS + (z * C::TH + y) * C::TW + x] = val;
  };
  auto store_staged = [&]() __attribute__((always_inline)) {
    __syncthreads();
    constexpr int QPR = C::TW / 4, NQ = C::COUT * C::TD * C::TH * QPR;      // float4 per row, per tile
#pragma unroll 4
    for (int q4 = tid; q4 < NQ; q4 += 256) {
      const int co = q4 / (C::TD * C::TH * QPR), rem = q4 % (C::TD * C::TH * QPR);
      const int row = rem / QPR, xq4 = rem % QPR;
      const int gz = oz0 + row / C::TH, gy = oy0 + row % C::TH, gx = ox0 + 4 * xq4;
      if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;     // Wo % 4 == 0: a float4 is inside or outside as a whole
      f32x4 val = *reinterpret_cast<const f32x4*>(os + co * OCS + row * C::TW + 4 * xq4);
      const size_t o = ((size_t)n * C::COUT + co) * out_plane + ((size_t)gz * p.Ho + gy) * p.Wo + gx;
      if (p.skip) val += *reinterpret_cast<const f32x4*>(p.skip + o);
      *reinterpret_cast<f32x4*>(p.out + o) = val;
    }
  };
  if (staged) __syncthreads();                     // every wave is done reading the input tile / weight fragments
  if constexpr (MODE == kDeconvS2) {
    // This wave owns output parities (pz, py) = (wave >> 1, wave & 1) and BOTH x parities
    // (accumulator halves cl = 0 / 1), so lane jn holds x = 2 xc and 2 xc + 1: one float2 store per
    // (channel, voxel pair) -> 16 lanes write 128 contiguous bytes.
    const int pz = (wave >> 1) & 1, py = wave & 1;
    if (staged) {
#pragma unroll
      for (int i = 0; i < C::NBC; ++i) {
        const int v = i * 16 + jn;
        if (v >= C::NVC) continue;
        const int z = 2 * (v / (C::CH * C::CW)) + pz, y = 2 * ((v / C::CW) % C::CH) + py, x = 2 * (v % C::CW);
#pragma unroll
        for (int m = 0; m < C::MB; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = m * 16 + kq * 4 + r;
            if (co < C::COUT) { stage_value(co, z, y, x, acc[i][m][r]); stage_value(co, z, y, x + 1, acc[C::NBC + i][m][r]); }
          }
      }
      store_staged();
      PHASE_MARK(6);
      PHASE_FLUSH;
      return;
    }
#pragma unroll
    for (int i = 0; i < C::NBC; ++i) {
      const int v = i * 16 + jn;
      if (v >= C::NVC) continue;
      const int z = 2 * (v / (C::CH * C::CW)) + pz, y = 2 * ((v / C::CW) % C::CH) + py;
      const int x = 2 * (v % C::CW);
      const int gz = oz0 + z, gy = oy0 + y, gx = ox0 + x;
      if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;      // Wo is even: gx + 1 < Wo too
      const size_t sp = ((size_t)gz * p.Ho + gy) * p.Wo + gx;
#pragma unroll
      for (int m = 0; m < C::MB; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = m * 16 + kq * 4 + r;
          if (co < C::COUT) {
            const float bsv = p.bias[co];
            float2 val = make_float2(acc[i][m][r] + bsv, acc[C::NBC + i][m][r] + bsv);
            if (p.relu) { val.x = fmaxf(val.x, 0.f); val.y = fmaxf(val.y, 0.f); }
            const size_t o = ((size_t)n * C::COUT + co) * out_plane + sp;
            if (p.skip) {
              const float2 sk = *reinterpret_cast<const float2*>(p.skip + o);
              val.x += sk.x; val.y += sk.y;
            }
            *reinterpret_cast<float2*>(p.out + o) = val;
          }
        }
      }
    }
  } else if constexpr (MODE == kConvS1Pair) {
    // rows 0-7: x shift 0, rows 8-15: x shift 1 -> lane quarter kq holds channels 4*(kq&1)+r at
    // x = 2*pair + (kq >> 1); quarters kq and kq+2 interleave into full 128-B runs per channel.
    const int sx = kq >> 1, cbase = 4 * (kq & 1);
    if (staged) {
#pragma unroll
      for (int j = 0; j < C::NBW; ++j) {
        const int v = (wave * C::NBW + j) * 16 + jn;
        if (v >= C::NVC) continue;
        const int z = v / (C::CH * C::CW), y = (v / C::CW) % C::CH, x = 2 * (v % C::CW) + sx;
#pragma unroll
        for (int r = 0; r < 4; ++r) stage_value(cbase + r, z, y, x, acc[j][0][r]);
      }
      store_staged();
      PHASE_MARK(6);
      PHASE_FLUSH;
      return;
    }
#pragma unroll
    for (int j = 0; j < C::NBW; ++j) {
      const int v = (wave * C::NBW + j) * 16 + jn;
      if (v >= C::NVC) continue;
      const int z = v / (C::CH * C::CW), y = (v / C::CW) % C::CH, x = 2 * (v % C::CW) + sx;
      const int gz = oz0 + z, gy = oy0 + y, gx = ox0 + x;
      if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;
      const size_t sp = ((size_t)gz * p.Ho + gy) * p.Wo + gx;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cbase + r;
        float val = acc[j][0][r] + p.bias[co];
        if (p.relu) val = fmaxf(val, 0.f);
        const size_t o = ((size_t)n * C::COUT + co) * out_plane + sp;
        if (p.skip) val += p.skip[o];
        p.out[o] = val;
      }
    }
  } else {
    if (staged) {
#pragma unroll
      for (int j = 0; j < C::NBW; ++j) {
        const int v = (wave * C::NBW + j) * 16 + jn;
        if (v >= C::NVC) continue;
        const int z = v / (C::CH * C::CW), y = (v / C::CW) % C::CH, x = v % C::CW;
#pragma unroll
        for (int m = 0; m < C::MB; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = m * 16 + kq * 4 + r;
            if (co < C::COUT) stage_value(co, z, y, x, acc[j][m][r]);
          }
      }
      store_staged();
      PHASE_MARK(6);
      PHASE_FLUSH;
      return;
    }
#pragma unroll
    for (int j = 0; j < C::NBW; ++j) {
      const int v = (wave * C::NBW + j) * 16 + jn;
      if (v >= C::NVC) continue;
      const int z = v / (C::CH * C::CW), y = (v / C::CW) % C::CH, x = v % C::CW;
      const int gz = oz0 + z, gy = oy0 + y, gx = ox0 + x;
      if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;
      const size_t sp = ((size_t)gz * p.Ho + gy) * p.Wo + gx;
#pragma unroll
      for (int m = 0; m < C::MB; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = m * 16 + kq * 4 + r;
          if (co < C::COUT) {
            float val = acc[j][m][r] + p.bias[co];
            if (p.relu) val = fmaxf(val, 0.f);
            const size_t o = ((size_t)n * C::COUT + co) * out_plane + sp;
            if (p.skip) val += p.skip[o];
            p.out[o] = val;
          }
        }
      }
    }
  }
  PHASE_MARK(6);
  PHASE_FLUSH;
}

// ---- layer table ---------------------------------------------------------------------------------
//                       mode      Cin Cout  TD TH  TW  CK
#ifndef V3D_L0_CFG
#define V3D_L0_CFG kConvS1Pair, 32, 8, 4, 8, 28, 4, 3
#endif
typedef ConvCfg<V3D_L0_CFG> L0;
// CostRegNet(16, 8) (the reference's signature default feat_dim = 16, lightningmodel.py:18): the exact-fp32 conv0 with 16 input
// channels; the split-bf16 / depth-march conv0 kernels run on the volume zero-extended to 32 channels with zero weights
typedef ConvCfg<kConvS1Pair, 16, 8, 4, 8, 28, 4, 3> L0_16;
#ifndef V3D_L1_CFG
#define V3D_L1_CFG kConvS2, 8, 16, 2, 4, 28, 4
#endif
typedef ConvCfg<V3D_L1_CFG> L1;
#ifndef V3D_L2_CFG
#define V3D_L2_CFG kConvS1, 16, 16, 4, 4, 28, 8
#endif
typedef ConvCfg<V3D_L2_CFG> L2;
typedef ConvCfg<kConvS2, 16, 32, 2, 7, 14, 4> L3;
typedef ConvCfg<kConvS1, 32, 32, 4, 7, 14, 8> L4;
typedef ConvCfg<kConvS2, 32, 64, 2, 4, 7, 8> L5;
typedef ConvCfg<kConvS1, 64, 64, 2, 4, 7, 16> L6;
typedef ConvCfg<kDeconvS2, 64, 32, 4, 8, 14, 16> L7;
#ifndef V3D_L8_CFG
#define V3D_L8_CFG kDeconvS2, 32, 16, 4, 8, 28, 8
#endif
typedef ConvCfg<V3D_L8_CFG> L8;
#ifndef V3D_L9_CFG
#define V3D_L9_CFG kDeconvS2, 16, 8, 4, 8, 28, 16, 3
#endif
typedef ConvCfg<V3D_L9_CFG> L9;

template <class C>
int launch_conv(const char* name, const float* in, const float* wp, const float* bias,
                const float* skip, float* out, int n, int Di, int Hi, int Wi, hipStream_t s) {
  ConvParams p;
  p.in = in; p.wp = wp; p.bias = bias; p.skip = skip; p.out = out; p.n = n;
  p.Di = Di; p.Hi = Hi; p.Wi = Wi;
  if (C::S1LIKE) { p.Do = Di; p.Ho = Hi; p.Wo = Wi; }
  else if (C::MODE == kConvS2) { p.Do = (Di - 1) / 2 + 1; p.Ho = (Hi - 1) / 2 + 1; p.Wo = (Wi - 1) / 2 + 1; }
  else { p.Do = 2 * Di; p.Ho = 2 * Hi; p.Wo = 2 * Wi; }
  p.ntz = (p.Do + C::TD - 1) / C::TD; p.nty = (p.Ho + C::TH - 1) / C::TH; p.ntx = (p.Wo + C::TW - 1) / C::TW;
  p.relu = 1;
  p.zy_order = 0;
  const long long blocks = (long long)n * p.ntz * p.nty * p.ntx;
  V3D_REQUIRE(blocks > 0 && blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "conv3d: bad grid");
  V3D_REQUIRE((long long)C::CK * Di * Hi * Wi < (1ll << 31), V3D_ERR_BAD_SHAPE,
              "conv3d: input volume too large for 32-bit tile offsets");
  {
    v3d::TimedScope ts(name, s);
    // (conv0 only: on conv2 the 40 extra staging registers cost more than the loads save: 0.37 -> 0.41 ms)
    constexpr bool kVecOk = C::MODE == kConvS1Pair && C::PF && C::TW % 4 == 0 && C::IW <= 61;
    const bool vec = kVecOk && Wi % 4 == 0 && (reinterpret_cast<size_t>(in) & 15) == 0;
    if constexpr (kVecOk) {
      if (vec) conv3d_mfma_kernel<C, true><<<(unsigned)blocks, 256, 0, s>>>(p);
      else conv3d_mfma_kernel<C, false><<<(unsigned)blocks, 256, 0, s>>>(p);
    } else {
      conv3d_mfma_kernel<C, false><<<(unsigned)blocks, 256, 0, s>>>(p);
    }
  }
  V3D_CHECK_LAUNCH("conv3d_mfma_kernel");
  return V3D_OK;
}


// what the fragment image of a layer depends on
struct TileDesc { int mode, ck; };
const TileDesc kTiles[10] = {{L0::MODE, L0::CK}, {L1::MODE, L1::CK}, {L2::MODE, L2::CK}, {L3::MODE, L3::CK}, {L4::MODE, L4::CK},
                             {L5::MODE, L5::CK}, {L6::MODE, L6::CK}, {L7::MODE, L7::CK}, {L8::MODE, L8::CK}, {L9::MODE, L9::CK}};

}  // namespace

size_t tile_image_floats(int layer, int in_channels) {
  const TileDesc T = kTiles[layer];
  const int cin = layer == 0 ? in_channels : kLayers[layer].cin, cout = kLayers[layer].cout;
  const bool pair = T.mode == kConvS1Pair;
  return (size_t)(cin / T.ck) * (9 * (pair ? 4 : 3)) * (T.ck / 4) * (pair ? 1 : (cout + 15) / 16) * 64;
}

// exact-fp32 fragment image of a layer for conv3d_mfma_kernel: [chunk][tap][4-channel step][16-row block][lane 64]
void pack_tile_image(int layer, int in_channels, const float* w, float* wp) {
  const TileDesc T = kTiles[layer];
  const int cin = layer == 0 ? in_channels : kLayers[layer].cin, cout = kLayers[layer].cout;
  const bool pair = T.mode == kConvS1Pair;
  const int MB = pair ? 1 : (cout + 15) / 16, C4 = T.ck / 4, nchunk = cin / T.ck;
  const int KXN = pair ? 4 : 3, NT = 9 * KXN;
  for (int chunk = 0; chunk < nchunk; ++chunk)
    for (int tap = 0; tap < NT; ++tap)
      for (int c4 = 0; c4 < C4; ++c4)
        for (int m = 0; m < MB; ++m)
          for (int lane = 0; lane < 64; ++lane) {
            const int row = m * 16 + (lane & 15);
            const int ci = chunk * T.ck + c4 * 4 + (lane >> 4);
            float v = 0.f;
            if (pair) {
              // row = x-shift * 8 + channel; virtual tap = (kz, ky, kx') with kx' in 0..3
              const int sx = row >> 3, co = row & 7, kzy = tap / 4, kx = tap % 4 - sx;
              if (kx >= 0 && kx <= 2) v = w[((size_t)co * cin + ci) * 27 + kzy * 3 + kx];
            } else if (row < cout) {
              // Conv3d weight [Co, Ci, 3,3,3]; ConvTranspose3d weight [Ci, Co, 3,3,3]
              v = w[T.mode == kDeconvS2 ? ((size_t)ci * cout + row) * 27 + tap : ((size_t)row * cin + ci) * 27 + tap];
            }
            wp[((((size_t)chunk * NT + tap) * C4 + c4) * MB + m) * 64 + lane] = v;
          }
}

int launch_conv_fp32(int layer, int in_channels, const float* in, const float* wp, const float* bias, const float* skip, float* out,
                     int n, int Di, int Hi, int Wi, hipStream_t s) {
  switch (layer) {
    case 0:
      if (in_channels == 16) return launch_conv<L0_16>("costreg_conv0", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
      return launch_conv<L0>("costreg_conv0", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 1: return launch_conv<L1>("costreg_conv1", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 2: return launch_conv<L2>("costreg_conv2", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 3: return launch_conv<L3>("costreg_conv3", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 4: return launch_conv<L4>("costreg_conv4", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 5: return launch_conv<L5>("costreg_conv5", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 6: return launch_conv<L6>("costreg_conv6", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 7: return launch_conv<L7>("costreg_conv7", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 8: return launch_conv<L8>("costreg_conv8", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
    case 9: return launch_conv<L9>("costreg_conv9", in, wp, bias, skip, out, n, Di, Hi, Wi, s);
  }
  return fail(V3D_ERR_BAD_ARG, "costreg: layer %d out of range", layer);
}

}  // namespace v3d
