// CostRegNet, conv0 as a tile kernel on split-bf16 matrix cores: the per-layer entry point's conv0 (v3d_costreg_layer_f32 with
// V3D_PRECISION_SPLIT_BF16; fp32 [n, 32, D, H, W] in, fp32 [n, 8, D, H, W] out).  The chain runs conv0 as a depth march
// (conv0z.hip) on the two weight images packed here.  costreg.hip is the map of the family.
//
// conv0 (32 -> 8 channels at full resolution) carries 68 % of the regulariser's MACs.  bf16 MFMA runs at 16x
// the fp32-MFMA rate, so every fp32 operand is split x = hi + lo into two bf16 values (hi = RNE(x),
// lo = RNE(x - hi): 16 mantissa bits together) and the product is evaluated as hi*hi + hi*lo + lo*hi with
// fp32 accumulation: 3 bf16 MFMAs (K = 32) replace 8 fp32 MFMAs (K = 4).  Measured error of this layer
// 7e-6 of max|out| (fp32 MFMA: 7e-7) and <= 1e-5 relative on the final depth (gate: 1e-4) -- DESIGN.md.
// Same pair-mode geometry as the fp32 kernel: rows = 2 x-shifts x 8 output channels; one MFMA covers the 4 x
// taps of a (kz, ky) kernel row (k = 8*kx' + ci) for a group of 8 input channels.  LDS holds the halo'd tile
// channel-last in 16-byte slots (8 bf16 of one voxel), one array for hi and one for lo, so a B fragment is
// a single ds_read_b128; A fragments (weights, split on the host) sit in LDS per channel group.
#include <type_traits>

#include "costreg.h"
#include "phase_timing.h"
#include "weight_pack.h"

PHASE_TIMING_UNIT(v3d_debug_conv0_phase_read)

namespace v3d {
namespace {

struct C0 {
  static constexpr int TD = 4, TH = 8, TW = 28, ID = TD + 2, IH = TH + 2, IW = TW + 2;
  static constexpr int NVOXI = ID * IH * IW;                 // 1800 voxels in the halo'd tile
  static constexpr int CG = 8, NCH = 32 / CG;                // channels per chunk, chunks
  static constexpr int SROWS = ID * IH;                      // 60 spatial rows (z, y) of IW voxels
  static constexpr int WU32 = 9 * 2 * 64 * 4;                // weight words per chunk (hi + lo fragments)
  static constexpr size_t LDS_BYTES = (size_t)NVOXI * 16 * 2 + (size_t)WU32 * 4 + 3 * 64 * 4;
  static_assert(WU32 % 256 == 0, "geometry");
};

// conv0's input loads are plain loads: with the non-temporal hint the halo rows a neighbouring tile reads a moment later
// were not kept in L2 (-DV3D_C0_NT_LOAD; the timings here and below were taken on this kernel's split-input variant, the
// chain's conv0 before conv0z.hip: 1.135 vs 1.09 ms per 64 views, two alternating builds on one box).
#ifdef V3D_C0_NT_LOAD
#define V3D_C0_LOAD(p) __builtin_nontemporal_load(p)
#else
#define V3D_C0_LOAD(p) (*(p))
#endif
#ifndef V3D_C0_ABLATE
#define V3D_C0_ABLATE 0      // developer ablation (scripts/ab_build.sh): 1 no MFMAs
#endif
// The kernel is written as a tile walk (v3d::xcd_tile_walk): with a grid of the workgroups the chip holds at once
// (-DV3D_C0_PERSIST) a workgroup walks tiles first + i, first + i + G, ... of its XCD's contiguous run and the chunk pipeline
// runs straight across tile boundaries (the first chunk of the next tile is requested during the last MFMA phase of the
// current one).  Measured equal to one tile per workgroup (1.09 vs 1.11 ms per 64 views) with 15 % more halo traffic
// (4.30 vs 3.74 GB fetched: the resident workgroups run in lock step and share less in L2), so the default grid is one
// workgroup per tile: the kernel is bound by the per-chunk chain load -> commit -> barrier -> MFMA with one chunk of
// prefetch (registers) and a single LDS buffer, not by tile turnover.
__global__ __launch_bounds__(256, 2) void conv0_bf16x2_kernel(ConvParams p) {
  constexpr int NT = 256, RPI = NT / 32, RPW = C0::TH / 4;      // threads (4 waves), staging rows per iteration, rows per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* const xh = reinterpret_cast<u32x4*>(smem);                           // [NVOXI] hi slots
  u32x4* const xl = xh + C0::NVOXI;                                           // [NVOXI] lo slots
  unsigned* const wsu = reinterpret_cast<unsigned*>(xl + C0::NVOXI);          // [WU32] weight fragments
  int* const rowd = reinterpret_cast<int*>(wsu + C0::WU32);                   // [64] first voxel of a spatial row in the tile
  int* const rowg2 = rowd + 64;                                               // [2][64] global offset of the row, per tile parity

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const size_t in_plane = (size_t)p.Di * p.Hi * p.Wi;
  constexpr int kRowOob = -2147483647 - 1;

  struct Tile { int n, oz0, oy0, ox0; };
  auto decode = [&](int t) __attribute__((always_inline)) {
    Tile q;
    const int tx = t % p.ntx; t /= p.ntx;
    int ty, tz;
    if (p.zy_order) { tz = t % p.ntz; t /= p.ntz; ty = t % p.nty; q.n = t / p.nty; }
    else { ty = t % p.nty; t /= p.nty; tz = t % p.ntz; q.n = t / p.ntz; }
    q.oz0 = tz * C0::TD; q.oy0 = ty * C0::TH; q.ox0 = tx * C0::TW;
    return q;
  };
  auto fill_rows = [&](const Tile& q, int par) __attribute__((always_inline)) {
    if (tid < 64) {
      const int rz = tid / C0::IH, ry = tid % C0::IH;
      const int gz = q.oz0 - 1 + rz, gy = q.oy0 - 1 + ry;
      const bool ok = tid < C0::SROWS && gz >= 0 && gz < p.Di && gy >= 0 && gy < p.Hi;
      rowg2[par * 64 + tid] = ok ? (gz * p.Hi + gy) * p.Wi + q.ox0 - 1 : kRowOob;
    }
  };
  const v3d::TileWalk walk = v3d::xcd_tile_walk(p.n * p.ntz * p.nty * p.ntx);   // neighbouring tiles (shared halo) on one XCD's L2
  if (walk.t >= walk.end) return;
  Tile cur = decode(walk.t);
  if (tid < 64) {
    const int rz = tid / C0::IH, ry = tid % C0::IH;
    rowd[tid] = tid < C0::SROWS ? (rz * C0::IH + ry) * C0::IW : -1;
  }
  fill_rows(cur, 0);
  __syncthreads();

  // MFMA role: wave w owns output rows y = 2w, 2w+1 for all TD planes; one column block = the 14 x pairs of a row
  // (lanes 14, 15 idle), so an input row fetched from LDS feeds up to 3 output planes (z reuse).
  static_assert(C0::TH == 8 && C0::TW == 28, "wave -> row mapping");
  constexpr int NACC = C0::TD * RPW;
  f32x4 acc[NACC];

  // staging role: 32 lanes = x of one spatial row, 8 rows per iteration, 8 channels per lane
  const int grp = tid >> 5, lx = tid & 31;
  const bool xok = lx < C0::IW;
  constexpr int NITS_F = (C0::SROWS + RPI - 1) / RPI;           // 60 rows x 8 channels
  constexpr int NWQ = (C0::WU32 / 4 + NT - 1) / NT;             // 16-byte weight loads per thread
  float pre[NITS_F][C0::CG];
  u32x4 wreg[NWQ];
  // The loads of the next chunk are issued in three parts between the MFMA groups of the current chunk: the
  // vector-memory pipe takes ~16 cycles per 1 KB instruction, which would otherwise stall the wave in front of
  // its MFMAs for the whole batch (measured 3.3k cycles per chunk).
  auto issue_part = [&](const Tile& q, int par, int chunk, auto part_c) __attribute__((always_inline)) {
    constexpr int part = decltype(part_c)::value;
    const int* const rowg = rowg2 + par * 64;
    const int sgx = q.ox0 - 1 + lx;
    const bool xin = xok && sgx >= 0 && sgx < p.Wi;
    constexpr int per = (NITS_F + 2) / 3;
    const float* inc = p.in + ((size_t)q.n * 32 + (size_t)chunk * C0::CG) * in_plane + lx;
#pragma unroll
    for (int it = part * per; it < (part + 1) * per && it < NITS_F; ++it) {
      const int g = rowg[min(it * RPI + grp, 63)];
#pragma unroll
      for (int c = 0; c < C0::CG; ++c) pre[it][c] = (g != kRowOob && xin) ? V3D_C0_LOAD(inc + (size_t)c * in_plane + g) : 0.f;
    }
    const u32x4* wc = reinterpret_cast<const u32x4*>(p.wp) + (size_t)chunk * (C0::WU32 / 4) + tid;
    constexpr int wper = (NWQ + 2) / 3;
#pragma unroll
    for (int i = part * wper; i < (part + 1) * wper && i < NWQ; ++i)
      wreg[i] = (i * NT + tid < C0::WU32 / 4) ? wc[i * NT] : (u32x4){0u, 0u, 0u, 0u};
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NITS_F; ++it) {
      const int d = rowd[min(it * RPI + grp, 63)];
      if (d >= 0 && xok) {
        unsigned h[8], l[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          h[c] = bf16_rne(pre[it][c]);
          l[c] = bf16_rne(pre[it][c] - __uint_as_float(h[c] << 16));
        }
        xh[d + lx] = (u32x4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        xl[d + lx] = (u32x4){l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
      }
    }
#pragma unroll
    for (int i = 0; i < NWQ; ++i)
      if (i * NT + tid < C0::WU32 / 4) reinterpret_cast<u32x4*>(wsu)[i * NT + tid] = wreg[i];
  };
  // one ky slice of the 27 taps: the 3 kz weight fragments stay in registers, every input row read from LDS feeds
  // up to 3 output planes
  auto mfma_ky = [&](int ky) __attribute__((always_inline)) {
    const u32x4* wf = reinterpret_cast<const u32x4*>(wsu) + lane;
    bf16x8 a_hi[3], a_lo[3];
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
      a_hi[kz] = __builtin_bit_cast(bf16x8, wf[((kz * 3 + ky) * 2) * 64]);
      a_lo[kz] = __builtin_bit_cast(bf16x8, wf[((kz * 3 + ky) * 2 + 1) * 64]);
    }
#pragma unroll
    for (int yy = 0; yy < RPW; ++yy) {
      const int rowbase = (wave * RPW + yy + ky) * C0::IW + 2 * jn + kq;
#pragma unroll
      for (int iz = 0; iz < C0::ID; ++iz) {
        const bf16x8 b_hi = __builtin_bit_cast(bf16x8, xh[rowbase + iz * C0::IH * C0::IW]);
        const bf16x8 b_lo = __builtin_bit_cast(bf16x8, xl[rowbase + iz * C0::IH * C0::IW]);
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const int z = iz - kz;
          if (z >= 0 && z < C0::TD) acc[z * RPW + yy] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[kz], b_hi, acc[z * RPW + yy], 0, 0, 0);
        }
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const int z = iz - kz;
          if (z >= 0 && z < C0::TD) acc[z * RPW + yy] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi[kz], b_lo, acc[z * RPW + yy], 0, 0, 0);
        }
#pragma unroll
        for (int kz = 0; kz < 3; ++kz) {
          const int z = iz - kz;
          if (z >= 0 && z < C0::TD) acc[z * RPW + yy] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo[kz], b_hi, acc[z * RPW + yy], 0, 0, 0);
        }
      }
    }
  };

  // The bias reaches the epilogue through SGPRs: a per-lane vector load there makes the compiler wait for vmcnt(0) in front
  // of every conditionally stored accumulator, i.e. for the next tile's prefetch and for the stores just issued.
  float sbias[8];                          // wave-uniform addresses: scalar loads, eight SGPRs for the whole kernel
#pragma unroll
  for (int r = 0; r < 8; ++r) sbias[r] = p.bias[r];

  PHASE_DECL;
  issue_part(cur, 0, 0, std::integral_constant<int, 0>{});
  issue_part(cur, 0, 0, std::integral_constant<int, 1>{});
  issue_part(cur, 0, 0, std::integral_constant<int, 2>{});
  PHASE_MARK(0);
  int par = 0;
#pragma unroll 1
  for (int t = walk.t; t < walk.end; t += walk.step, par ^= 1) {
    const int tn = t + walk.step;
    const bool has_next = tn < walk.end;
    const Tile nxt = decode(has_next ? tn : t);
    // the row table of the next tile: written now, first read in the MFMA phase of this tile's last chunk (several barriers
    // later); its previous content (tile t - step) was last read in tile t - step's chunk 2
    if (has_next) fill_rows(nxt, par ^ 1);
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int chunk = 0; chunk < C0::NCH; ++chunk) {
      __syncthreads();
      PHASE_MARK(1);
      commit();
      PHASE_MARK(2);
      __syncthreads();
      PHASE_MARK(3);
      const bool last = chunk + 1 == C0::NCH;
      const bool more = !last || has_next;
      const Tile& lt = last ? nxt : cur;                  // tile / table / chunk the next staging round belongs to
      const int lpar = last ? par ^ 1 : par, lchunk = last ? 0 : chunk + 1;
      if (more) issue_part(lt, lpar, lchunk, std::integral_constant<int, 0>{});
      if (V3D_C0_ABLATE != 1) mfma_ky(0);
      if (more) issue_part(lt, lpar, lchunk, std::integral_constant<int, 1>{});
      if (V3D_C0_ABLATE != 1) mfma_ky(1);
      if (more) issue_part(lt, lpar, lchunk, std::integral_constant<int, 2>{});
      if (V3D_C0_ABLATE != 1) mfma_ky(2);
      PHASE_MARK(5);
    }

    // epilogue: rows 0-7 = x shift 0, rows 8-15 = x shift 1: lane (kq, jn) holds channels 4 (kq & 1) .. +3 of voxel
    // x = 2 jn + (kq >> 1).
    const int n = cur.n, oz0 = cur.oz0, oy0 = cur.oy0, ox0 = cur.ox0;
    // fp32 output: the tile goes through LDS ([co][z][y][28 x], co stride padded by 4 floats against bank conflicts)
    // so that it leaves as 16-byte row segments instead of 32 4-byte stores per lane.
    constexpr int OCS = C0::TD * C0::TH * C0::TW + 4;
    float* const os = reinterpret_cast<float*>(smem);
    __syncthreads();                 // every wave is done reading the input tile
    {
      const int sx = kq >> 1, cbase = 4 * (kq & 1);
      float bias[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) bias[r] = lane_select(kq & 1, sbias[4 + r], sbias[r]);
      if (jn < C0::TW / 2) {
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
          const int row = (j / RPW) * C0::TH + wave * RPW + j % RPW;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float val = acc[j][r] + bias[r];
            if (p.relu) val = fmaxf(val, 0.f);
            os[(cbase + r) * OCS + row * C0::TW + 2 * jn + sx] = val;
          }
        }
      }
    }
    __syncthreads();
    const size_t out_plane = (size_t)p.Do * p.Ho * p.Wo;
    constexpr int QPR = C0::TW / 4, NQ = 8 * C0::TD * C0::TH * QPR;      // float4 per row, per tile
#pragma unroll
    for (int k = 0; k < (NQ + NT - 1) / NT; ++k) {
      const int i = k * NT + tid;
      if (i >= NQ) break;
      const int co = i / (C0::TD * C0::TH * QPR), rem = i % (C0::TD * C0::TH * QPR);
      const int row = rem / QPR, q = rem % QPR;
      const int gz = oz0 + row / C0::TH, gy = oy0 + row % C0::TH, gx = ox0 + 4 * q;
      if (gz >= p.Do || gy >= p.Ho || gx >= p.Wo) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(os + co * OCS + row * C0::TW + 4 * q);
      const size_t o = ((size_t)n * 8 + co) * out_plane + ((size_t)gz * p.Ho + gy) * p.Wo + gx;
      if (gx + 3 < p.Wo && (p.Wo & 3) == 0) {
        if (p.skip) { const f32x4 sk = *reinterpret_cast<const f32x4*>(p.skip + o); v += sk; }
        *reinterpret_cast<f32x4*>(p.out + o) = v;
      } else {
        for (int e = 0; e < 4 && gx + e < p.Wo; ++e) p.out[o + e] = v[e] + (p.skip ? p.skip[o + e] : 0.f);
      }
    }
    PHASE_MARK(6);
    cur = nxt;
  }
  PHASE_FLUSH;
}

}  // namespace

int launch_conv0_bf16(const float* in, const float* wbf, const float* bias, const float* skip, float* out, int n, int Di, int Hi,
                      int Wi, hipStream_t s) {
  ConvParams p;
  p.in = in; p.wp = wbf; p.bias = bias; p.skip = skip; p.out = out; p.n = n;
  p.Di = Di; p.Hi = Hi; p.Wi = Wi; p.Do = Di; p.Ho = Hi; p.Wo = Wi;
  p.ntz = (Di + C0::TD - 1) / C0::TD; p.nty = (Hi + C0::TH - 1) / C0::TH; p.ntx = (Wi + C0::TW - 1) / C0::TW;
  p.relu = 1;
  p.zy_order = tile_order(p.ntx, p.nty);
  const long long blocks = (long long)n * p.ntz * p.nty * p.ntx;
  V3D_REQUIRE(blocks > 0 && blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "conv0: bad grid");
  V3D_REQUIRE((long long)8 * Di * Hi * Wi < (1ll << 31), V3D_ERR_BAD_SHAPE, "conv0: input volume too large");
  static bool lds_opted[64] = {};
  if (const int rc = opt_in_dynamic_lds((const void*)conv0_bf16x2_kernel, (int)C0::LDS_BYTES, lds_opted); rc != V3D_OK) return rc;
  {
    TimedScope ts("costreg_conv0", s);
#ifdef V3D_C0_PERSIST       // developer A/B: 512 resident workgroups walking their tiles (same time, 15 % more halo traffic)
    const unsigned grid = persistent_grid(blocks, 2);        // 76.8 KB of LDS: two workgroups per CU
#else
    const unsigned grid = (unsigned)((blocks + 7) / 8 * 8);       // one tile per workgroup: the walk has a single step
#endif
    conv0_bf16x2_kernel<<<grid, 256, C0::LDS_BYTES, s>>>(p);
  }
  V3D_CHECK_LAUNCH("conv0_bf16x2_kernel");
  return V3D_OK;
}

// conv0 in pair mode, lane (kx', row): row = x shift * 8 + co, kx = kx' - x shift of the 4-wide window; 0 where the shifted
// kernel does not reach and for input channels the net does not have (16 input channels: chunks 2, 3 carry zero weights)
static float conv0_pair_weight(const float* w, int in_channels, int lane, int kzy, int ci) {
  const int row = lane & 15, kxp = lane >> 4, sx = row >> 3, co = row & 7, kx = kxp - sx;
  return kx >= 0 && kx <= 2 && ci < in_channels ? w[((size_t)co * in_channels + ci) * 27 + kzy * 3 + kx] : 0.f;
}

// split-bf16 image of conv0: [chunk 4][kzy 9][hi, lo][lane 64][4 words].  Consumed by conv0_bf16x2_kernel and by the chain's
// conv0, conv0z_kernel<false> (conv0z.hip)
static_assert(kConv0SplitFloats == (size_t)C0::NCH * C0::WU32, "conv0 image size");
void pack_conv0_split(const float* w, int in_channels, unsigned* wb) {
  for (int chunk = 0; chunk < C0::NCH; ++chunk)
    for (int kzy = 0; kzy < 9; ++kzy)
      for (int lane = 0; lane < 64; ++lane) {
        float v[8];
        for (int e = 0; e < 8; ++e) v[e] = conv0_pair_weight(w, in_channels, lane, kzy, chunk * 8 + e);
        unsigned* dst = wb + ((size_t)chunk * 9 + kzy) * 2 * kLoWords + lane * 4;
        v3d::split_bf16x8(v, dst, dst + kLoWords);
      }
}

// exact-fp32 image of conv0, consumed by conv0z_kernel<true> alone (conv0z.hip; v_mfma_f32_16x16x4_f32, pair mode): [chunk 4][kz * 3 + ky][channel 8]
// [lane 64]; lane (kq, m): row m = x shift * 8 + co, k = x tap kq of the 4-wide window
void pack_conv0_f32(const float* w, int in_channels, float* wf) {
  for (int chunk = 0; chunk < 4; ++chunk)
    for (int kzy = 0; kzy < 9; ++kzy)
      for (int e = 0; e < 8; ++e)
        for (int lane = 0; lane < 64; ++lane)
          wf[(((size_t)chunk * 9 + kzy) * 8 + e) * 64 + lane] = conv0_pair_weight(w, in_channels, lane, kzy, chunk * 8 + e);
}

}  // namespace v3d
