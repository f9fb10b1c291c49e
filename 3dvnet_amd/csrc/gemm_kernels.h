// What the translation units of the gather-GEMM share (gemm_gather.hip is the map of the family): the launch parameters, ONE
// statement of every piece the kernels have in common -- the split-bf16 product, the swizzled hi/lo activation tile (commit and
// read), the row map, the weight-fragment load, the GroupNorm statistics --, both epilogues, and every unit's launcher.
//
// Orientation: D[co, row].  The A operand of a matrix instruction is the weight fragment (packed on the host, v3d_gemm_pack),
// the B operand the gathered activations; lane (kq = lane >> 4, jn = lane & 15) holds channels 4 kq .. 4 kq + 3 of row jn of a
// 16 x 16 block.  Each wave owns all NB row blocks x MBW channel blocks (16 outputs each; N <= 64 MBW) of the tile, so the
// per-row GroupNorm (16-channel groups == one channel block, scenemodeling.py:98-104) needs only two cross-lane shuffles.
// Split bf16: operands are split x = hi + lo into two bf16 values (16 mantissa bits together) and a product block is hi*hi +
// hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- 3 bf16 MFMAs (K = 32) instead of 8 fp32 MFMAs (K = 4),
// 5.3x the matrix rate at ~7e-6 relative layer error (the depth gate is 1e-4).
//   * activation tile in LDS: [hi, lo][row][4 k groups of 8 bf16] (64-byte rows, the lo array `lo_rows` rows behind the hi
//     array), the 16-byte k-group slot XOR-swizzled by bit 3 of the row: every ds_read_b128 lane group hits 16 distinct slots;
//   * packed weight image per (segment, K chunk of 32): [hi, lo][MB = 4 MBW channel blocks][64 lanes][4 words]; lane l holds
//     output co = mb*16 + (l & 15), k = chunk*32 + 8*(l >> 4) + e (e = 0..7, two bf16 per word).
// Exact fp32 (the one-step kernel only): activation tile [row][kXS floats] (row stride 34 = conflict-free for the 4 k-lanes x
// 16 row-lanes), weight slab of a (segment, chunk) [8 k4][MB][64 lanes] floats through LDS, for v_mfma_f32_16x16x4_f32.
#pragma once
#include "bf16_split.h"
#include "v3d_common.h"

namespace v3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxSeg = 27;
constexpr int kKC = 32;      // K chunk
constexpr int kXS = kKC + 2; // LDS row stride of the fp32 activation tile

struct Seg {
  const float* src;
  const int* idx;   // row map or null (identity)
  int ld;           // row stride of src in floats
};

struct GemmParams {
  Seg seg[kMaxSeg];
  int n_seg, M, N, K, KP;        // K real columns per segment, KP = K rounded up to kKC
  int group_len;                 // > 0: conv1d row map (segment s reads row m + s - n_seg/2 of its group)
  int relu_in;
  const float* wp;               // packed [seg][KP/32][8][MB][64]
  const float* bias;             // [N] or null
  const float* gn_w; const float* gn_b; float gn_eps;   // row GroupNorm over 16-channel groups (null = off)
  int gn8;                                              // ... over 8-channel groups instead (use_gn == 8)
  const float* residual; int ld_res;
  int relu_out;
  float* pool; const int* pool_idx; int ld_pool;        // scatter-max target (null = off)
  float* out; int ld_out;                               // null = do not store
};

// Launchers (nb: 16-row blocks per tile; blocks: tiles): each holds its kernel's instantiation switch; launch_gemm() refuses a
// combination the switch has no kernel for, launches, and names the kernel that ran in a launch error
int launch_dense(const GemmParams& p, int MBW, int nb, bool bf16, unsigned blocks, hipStream_t s);                    // gemm_dense.hip
int launch_rounds(const GemmParams& p, int MBW, int nb, unsigned blocks, hipStream_t s);                              // gemm_sparse.hip
int launch_pipe(const GemmParams& p, int MBW, int nb, int loaders, int min_blocks, unsigned blocks, hipStream_t s);   // gemm_sparse.hip
int launch_conv1d(const GemmParams& p, int MBW, int nb, unsigned blocks, hipStream_t s);                              // gemm_conv1d.hip
typedef void (*GemmKernel)(GemmParams);
inline int launch_gemm(GemmKernel k, const char* name, const GemmParams& p, unsigned blocks, unsigned threads, hipStream_t s) {
  V3D_REQUIRE(k, V3D_ERR_BAD_ARG, "%s: no instantiation for this channel-block count and tile shape", name);
  k<<<blocks, threads, 0, s>>>(p);
  V3D_CHECK_LAUNCH(name);
  return V3D_OK;
}

__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
  // order-independent max for mixed-sign floats; target initialised to -inf
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

template <int NB, int MBW>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NB][MBW]) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int m = 0; m < MBW; ++m) acc[nb][m] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// The split-bf16 product of one (channel block, row block, K chunk): hi*hi, hi*lo, lo*hi, in this order in every kernel
__device__ __forceinline__ void mfma_split3(bf16x8 a_hi, bf16x8 a_lo, bf16x8 b_hi, bf16x8 b_lo, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_hi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_hi, b_lo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_lo, b_hi, acc, 0, 0, 0);
}

// B fragments of a lane: k group kq of tile row `row`, hi and lo, through the swizzle of the layout above
__device__ __forceinline__ void read_b(const u32x4* tile, int lo_rows, int row, int kq, bf16x8& b_hi, bf16x8& b_lo) {
  const int bslot = kq ^ (((row >> 3) & 1) * 3);
  b_hi = __builtin_bit_cast(bf16x8, tile[row * 4 + bslot]);
  b_lo = __builtin_bit_cast(bf16x8, tile[(lo_rows + row) * 4 + bslot]);
}

__device__ __forceinline__ void relu4(f32x4& v) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }

// A staging thread's gathered k = sc4 .. sc4 + 3 of tile row `row` (half of the 8-wide k group sc4 / 8): optional ReLU, split,
// and the two 8-byte stores into the hi and lo arrays
__device__ __forceinline__ void commit_split(u32x4* tile, int lo_rows, int row, int sc4, f32x4 v, int relu_in) {
  if (relu_in) relu4(v);
  const int kg = sc4 >> 3, half = (sc4 >> 2) & 1;
  const int slot = kg ^ (((row >> 3) & 1) * 3);
  u32x2 hp, lp;
  split4(v.x, v.y, v.z, v.w, hp, lp);      // bf16_split.h: 12 vector instructions per four values
  u32x2* xh2 = reinterpret_cast<u32x2*>(tile);
  xh2[(row * 4 + slot) * 2 + half] = hp;
  xh2[((lo_rows + row) * 4 + slot) * 2 + half] = lp;
}

// Source row of output row m in segment s: the conv1d tap inside its group, the segment's row map, or m itself; -1 = zero row
// (a tap that leaves its group, an absent neighbour, a row behind M)
__device__ __forceinline__ int source_row(const GemmParams& p, int s, int m) {
  if (m >= p.M) return -1;
  if (p.group_len > 0) {
    const int h = m % p.group_len + s - p.n_seg / 2;
    return (h >= 0 && h < p.group_len) ? m + s - p.n_seg / 2 : -1;
  }
  const int* idx = p.seg[s].idx;
  return idx ? idx[m] : m;
}

// The hi and lo weight fragments of a wave's MBW channel blocks for step (segment, K chunk), from the packed image (L2-resident)
// straight into registers: they are never shared between waves.  wbase = fragment_base(): the wave's and lane's place inside
// a step's slab, which a kernel computes once.
template <int MBW>
__device__ __forceinline__ const u32x4* fragment_base(const float* wp, int wave, int lane) {
  return reinterpret_cast<const u32x4*>(wp) + wave * MBW * 64 + lane;
}
template <int MBW>
__device__ __forceinline__ void load_fragments(const u32x4* wbase, int seg, int kc, int nkc, u32x4 (&a)[2 * MBW]) {
  constexpr int kWslab = 4 * MBW * 16 * kKC, MB = 4 * MBW;      // packed floats per (segment, K chunk)
  const u32x4* w = wbase + (size_t)(seg * nkc + kc) * (kWslab / 4);
#pragma unroll
  for (int m = 0; m < MBW; ++m) {
    a[m] = w[m * 64];
    a[MBW + m] = w[(MB + m) * 64];
  }
}

// GroupNorm statistics of a row's channel group: the 16 channels of the block = 4 registers x 4 lane quarters (8-channel groups
// -- SparseUNet(dims[0] = 32, 4 groups), the reference's feat_dim = 16 -- are the lane quarter pairs (0, 1) and (2, 3))
__device__ __forceinline__ void group_norm4(const float (&v)[4], int gn8, float eps, float& mean, float& rstd) {
  const float ginv = gn8 ? 1.f / 8.f : 1.f / 16.f;
  float sum = v[0] + v[1] + v[2] + v[3];
  sum += __shfl_xor(sum, 16);
  if (!gn8) sum += __shfl_xor(sum, 32);
  mean = sum * ginv;
  float sq = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) sq += (v[r] - mean) * (v[r] - mean);
  sq += __shfl_xor(sq, 16);
  if (!gn8) sq += __shfl_xor(sq, 32);
  rstd = 1.f / sqrtf(sq * ginv + eps);      // biased variance (torch GN)
}

// ---- epilogue shared by the GEMM kernels: bias -> GroupNorm -> residual -> ReLU -> scatter-max (order-independent) -> store ----
template <int MBW, int NB>
__device__ __forceinline__ void gemm_epilogue_generic(const GemmParams& p, f32x4 (&acc)[NB][MBW], int m0, int wave, int kq, int jn) {
  // lane (kq, jn) holds channels co0 .. co0+3 of row m0 + nb*16 + jn
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int m = m0 + nb * 16 + jn;
#pragma unroll
    for (int mw = 0; mw < MBW; ++mw) {
      const int co0 = (wave * MBW + mw) * 16 + kq * 4;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[nb][mw][r] + ((p.bias && co0 + r < p.N) ? p.bias[co0 + r] : 0.f);
      if (p.gn_w) {
        float mean, rstd;
        group_norm4(v, p.gn8, p.gn_eps, mean, rstd);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (co0 + r < p.N) v[r] = (v[r] - mean) * rstd * p.gn_w[co0 + r] + p.gn_b[co0 + r];
      }
      if (m < p.M && co0 < p.N) {
        if (p.residual) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (co0 + r < p.N) v[r] += p.residual[(size_t)m * p.ld_res + co0 + r];
        }
        if (p.relu_out) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (p.pool) {
          float* pr = p.pool + (size_t)p.pool_idx[m] * p.ld_pool + co0;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (co0 + r < p.N) atomic_max_float(pr + r, v[r]);
        }
        if (p.out) {
          float* o = p.out + (size_t)m * p.ld_out + co0;
          if (co0 + 3 < p.N && (p.ld_out % 4 == 0)) {
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (co0 + r < p.N) o[r] = v[r];
          }
        }
      }
    }
  }
}

// The same epilogue for the shapes every hot caller has (N a multiple of 16, 16-byte aligned rows of `out` / `residual`, no
// scatter-max): the generic code above loads bias / GroupNorm affine / residual one float at a time inside the (row block,
// channel block) loops and waits for each -- the compiler cannot move a load across the stores of the previous block -- which made
// the epilogue 28 k of the 46 k cycles of a PointNet layer's workgroup (scripts/micro/phase_dense_gemm.py) and ~10 % of a sparse
// convolution.  Here the per-channel constants are read once as float4, the residual rows of the whole tile are requested before
// the first is used, and nothing but the stores is predicated.  Same arithmetic, same order (group_norm4 is the statistics of
// both): bit-identical.
template <int MBW, int NB>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[NB][MBW], int m0, int wave, int kq, int jn) {
  const bool fast = p.N % 16 == 0 && !p.pool && (!p.out || (p.ld_out % 4 == 0 && (reinterpret_cast<size_t>(p.out) & 15) == 0)) &&
                    (!p.residual || (p.ld_res % 4 == 0 && (reinterpret_cast<size_t>(p.residual) & 15) == 0)) &&
                    (!p.bias || (reinterpret_cast<size_t>(p.bias) & 15) == 0) &&
                    (!p.gn_w || ((reinterpret_cast<size_t>(p.gn_w) & 15) == 0 && (reinterpret_cast<size_t>(p.gn_b) & 15) == 0));
  if (!fast) {
    gemm_epilogue_generic<MBW, NB>(p, acc, m0, wave, kq, jn);
    return;
  }
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 b4[MBW], gw4[MBW], gb4[MBW];
  int coc[MBW];
  bool cok[MBW];
#pragma unroll
  for (int mw = 0; mw < MBW; ++mw) {
    const int co0 = (wave * MBW + mw) * 16 + kq * 4;
    cok[mw] = co0 < p.N;
    coc[mw] = cok[mw] ? co0 : 0;                    // a channel block behind N reads block 0 and stores nothing
    b4[mw] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + coc[mw]) : zero4;
    if (!cok[mw]) b4[mw] = zero4;                   // (the generic code adds no bias there; the GroupNorm of such a block is never stored)
    gw4[mw] = p.gn_w ? *reinterpret_cast<const f32x4*>(p.gn_w + coc[mw]) : zero4;
    gb4[mw] = p.gn_w ? *reinterpret_cast<const f32x4*>(p.gn_b + coc[mw]) : zero4;
  }
  // the residual rows of four row blocks at a time are requested before the first is used (all of a 64-row tile)
  constexpr int G = NB < 4 ? NB : 4;
#pragma unroll
  for (int g0 = 0; g0 < NB; g0 += G) {
    f32x4 res[G][MBW];
    if (p.residual) {
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int m = m0 + (g0 + g) * 16 + jn, mc = m < p.M ? m : p.M - 1;
#pragma unroll
        for (int mw = 0; mw < MBW; ++mw)
          res[g][mw] = *reinterpret_cast<const f32x4*>(p.residual + (size_t)mc * p.ld_res + coc[mw]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int nb = g0 + g, m = m0 + nb * 16 + jn;
#pragma unroll
      for (int mw = 0; mw < MBW; ++mw) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[nb][mw][r] + b4[mw][r];
        if (p.gn_w) {
          float mean, rstd;
          group_norm4(v, p.gn8, p.gn_eps, mean, rstd);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (v[r] - mean) * rstd * gw4[mw][r] + gb4[mw][r];
        }
        if (p.residual) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += res[g][mw][r];
        }
        if (p.relu_out) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if (p.out && m < p.M && cok[mw])
          *reinterpret_cast<f32x4*>(p.out + (size_t)m * p.ld_out + coc[mw]) = (f32x4){v[0], v[1], v[2], v[3]};
      }
    }
  }
}

}  // namespace v3d
