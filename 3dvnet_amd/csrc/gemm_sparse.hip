// The small-M kernels of the sparse convolutions: the rounds kernel and the loader / matrix pipeline (gemm_gather.hip is the map
// of the family, gemm_kernels.h what its kernels share; gemm_gather_kernel, the one-step kernel, is gemm_dense.hip's).
#include "gemm_kernels.h"
#include "phase_timing.h"

PHASE_TIMING_UNIT(v3d_debug_sparse_gemm_phase_read)

using namespace v3d;

namespace {

// ---- the same GEMM in rounds of S (segment, K chunk) steps: the small-M kernel of the sparse convolutions ------------------
// gemm_gather_kernel moves ONE step per pair of barriers: a thread has one 16-byte gather (and its share of the weight slab)
// in flight, so a tile's time is (number of steps) x (a memory round trip): 27 offsets x K / 32 chunks -- 108 steps on the
// 128-channel level of the sparse U-Net, whose 3.5 k rows are 110 workgroups on 256 CUs (nothing else hides the latency).
// Here a round stages S steps' activation tiles at once (S gathers per thread in flight, one pair of barriers per round) and the
// weight fragments go from L2 straight into the registers of the wave that owns the channel block (they were never shared
// between waves; the LDS round trip of the slab is gone).  The neighbour-table column of every segment is read once into an
// LDS row table (the old kernel read it twice: activity scan + staging).  Same step order and MFMA order per accumulator:
// bit-identical to gemm_gather_kernel<MBW, NB, true>.
template <int MBW, int NB, int S>
__global__ __launch_bounds__(256) void gemm_gather_rounds_kernel(GemmParams p) {
  constexpr int kTM = 16 * NB, NPASS = (kTM + 31) / 32;
  constexpr int kTile = 2 * kTM * 4;                // 16-byte slots of one step's activation tile: [hi, lo][row][4 k groups]
  __shared__ __attribute__((aligned(16))) u32x4 xq[S * kTile];
  __shared__ int rowtab[kMaxSeg * kTM];
  __shared__ int s_act[kMaxSeg], s_list[kMaxSeg], s_nact;
  __shared__ int steptab[kMaxSeg * 8 + 2 * S];     // (segment << 8 | K chunk) of every step of the flat sequence, -1 behind its end

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  // rows are sorted by voxel key: a contiguous run of tiles per XCD keeps the neighbour rows a tile gathers in that XCD's L2
  const int m0 = xcd_contiguous_block() * kTM;
  const int nkc = p.KP / kKC;

  f32x4 acc[NB][MBW];
  zero_acc(acc);

  // ---- row table: source row of (segment, tile row), -1 = zero row; which segments does the tile need at all? ----------------
  if (tid < kMaxSeg) s_act[tid] = 0;
  __syncthreads();
  for (int e = tid; e < p.n_seg * kTM; e += 256) {
    const int sg = e / kTM, row = e % kTM;
    const int v = source_row(p, sg, m0 + row);
    rowtab[e] = v;
    if (v >= 0 || p.seg[sg].idx == nullptr) s_act[sg] = 1;       // benign race: everybody writes the same value
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int sg = 0; sg < p.n_seg; ++sg) if (s_act[sg]) s_list[n++] = sg;
    s_nact = n;
  }
  __syncthreads();
  const int n_steps = s_nact * nkc;                 // flat (active segment, K chunk) sequence
  for (int f = tid; f < n_steps + 2 * S; f += 256) steptab[f] = f < n_steps ? (s_list[f / nkc] << 8) | (f % nkc) : -1;
  __syncthreads();
  // One source matrix for every segment (a sparse convolution: only the row maps differ): its pointer and row stride are read
  // once.  Otherwise they are looked up per step -- a scalar load from the kernel arguments behind an LDS read, ~500 cycles in
  // front of every gather (measured: 1.9 k cycles per round of four steps just to issue the gathers).
  bool one_src = true;
  for (int sg = 1; sg < p.n_seg; ++sg) one_src = one_src && p.seg[sg].src == p.seg[0].src && p.seg[sg].ld == p.seg[0].ld;
  const float* const src0 = p.seg[0].src;
  const int ld0 = p.seg[0].ld;
  PHASE_DECL;

  // staging role: 8 lanes x float4 cover the 32 columns of one row; 32 rows per pass
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  f32x4 xr[S][NPASS];
  u32x4 afr[S][2 * MBW];
  int st[S];                                        // the steps of the round being issued (wave-uniform)
  auto load_steps = [&](int f0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) st[j] = __builtin_amdgcn_readfirstlane(steptab[f0 + j]);
  };
  auto issue_x = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (st[j] >= 0) {
        const int sg = st[j] >> 8, col = (st[j] & 255) * kKC + sc4;
        const float* const src = one_src ? src0 : p.seg[sg].src;
        const int ld = one_src ? ld0 : p.seg[sg].ld;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
          const int row = srow + 32 * i;
          const int r = row < kTM ? rowtab[sg * kTM + row] : -1;
          xr[j][i] = (r >= 0 && col < p.K) ? *reinterpret_cast<const f32x4*>(src + (size_t)r * ld + col)
                                           : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  };
  const u32x4* const wbase = fragment_base<MBW>(p.wp, wave, lane);
  auto issue_a = [&](int stj, u32x4 (&a)[2 * MBW]) __attribute__((always_inline)) {
    if (stj >= 0) load_fragments<MBW>(wbase, stj >> 8, stj & 255, nkc, a);
  };
  auto commit = [&](int f0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (f0 + j < n_steps) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
          const int row = srow + 32 * i;
          if (row < kTM) commit_split(xq + j * kTile, kTM, row, sc4, xr[j][i], p.relu_in);
        }
      }
    }
  };

  load_steps(0);
  issue_x();
#pragma unroll
  for (int j = 0; j < S; ++j) issue_a(st[j], afr[j]);
  PHASE_MARK(0);
#pragma unroll 1
  for (int f0 = 0; f0 < n_steps; f0 += S) {
    __syncthreads();                 // the previous round's MFMAs are done with the activation tiles
    PHASE_MARK(1);
    commit(f0);
    PHASE_MARK(2);
    __syncthreads();
    PHASE_MARK(3);
    load_steps(f0 + S);
    issue_x();                       // the next round's gathers fly during this round's MFMAs
    PHASE_MARK(4);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (f0 + j < n_steps) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          bf16x8 b_hi, b_lo;
          read_b(xq + j * kTile, kTM, nb * 16 + jn, kq, b_hi, b_lo);
#pragma unroll
          for (int m = 0; m < MBW; ++m)
            mfma_split3(__builtin_bit_cast(bf16x8, afr[j][m]), __builtin_bit_cast(bf16x8, afr[j][MBW + m]), b_hi, b_lo, acc[nb][m]);
        }
      }
      issue_a(st[j], afr[j]);        // this step's fragment registers are free: the next round's step j takes them
    }
    PHASE_MARK(5);
  }
  gemm_epilogue<MBW, NB>(p, acc, m0, wave, kq, jn);
  PHASE_MARK(6);
  PHASE_FLUSH;
}

// ---- the sparse convolution as a loader / matrix pipeline (round 5) ----------------------------------------------------------
// Phase counters of the rounds kernel on the cfg3 U-Net (13 434 rows x 128 channels, 32-row tiles): of 154 k cycles per
// workgroup 38 k wait for the gathers, 49 k ISSUE them (the CU's vector-memory path is busy with the 1.77 MB of weight
// fragments every tile streams: 64 KB per round) and 49 k are the matrix instructions + the wait for those fragments --
// nothing overlaps, because one wave does all three in turn and its loads retire in order.  Here the roles are separate waves
// with separate load queues: the loader waves (4 or 8 of them behind the four matrix waves) gather the neighbour rows U rounds
// ahead (registers), split them and fill a 2-slot LDS ring; waves 0..3 keep the weight fragments of the next AD - 1 rounds in
// flight and run the matrix instructions; one barrier per round of S steps.  64-row tiles halve the weight stream per row (one workgroup per CU at 13 k rows).  Every load is
// unconditional (absent rows read row 0 and are masked in registers; rounds behind the end repeat step 0 and are not
// multiplied), so the compiler's s_waitcnt counting is exact and the prefetch distance survives.  Same step order and MFMA
// order per accumulator as gemm_gather_kernel<MBW, NB, true>: bit-identical.
// Step sequence of a tile: the active segments in ascending order x the K chunks, kept as a bit mask + a chunk counter in
// scalar registers (an LDS step table costs an LDS round trip + v_readfirstlane in front of every load address).
struct StepIter {
  unsigned mask;   // active segments not yet finished (wave-uniform)
  int kc;
  __device__ __forceinline__ bool next(int nkc, int& sg, int& k) {   // false behind the end (sg = k = 0 then)
    const bool ok = mask != 0;
    sg = ok ? __builtin_ctz(mask) : 0;
    k = ok ? kc : 0;
    const bool wrap = kc + 1 == nkc;
    mask = (ok && wrap) ? (mask & (mask - 1)) : mask;
    kc = ok ? (wrap ? 0 : kc + 1) : kc;
    return ok;
  }
};

#ifndef V3D_PIPE_ABLATE
#define V3D_PIPE_ABLATE 0     // developer ablations (scripts/micro/sparse_ablate.sh): 1 no MFMAs, 2 no fragment loads, 3 no gathers, 4 no split / LDS writes
#endif
// NL: loader waves (4 or 8); AD: depth of the weight-fragment ring of the matrix waves (fragments of AD - 1 rounds in flight)
template <int MBW, int NB, int NL, int MINB>
__global__ __launch_bounds__(256 + 64 * NL, MINB) void gemm_gather_pipe_kernel(GemmParams p) {
  constexpr int kTM = 16 * NB, S = 2, U = 4, NT = 256 + 64 * NL, AD = 2;
  constexpr int RPP = NL * 8;                       // rows per loader pass: 8 threads x 16 B = one 128-byte row slice
  constexpr int NPASS = (kTM + RPP - 1) / RPP;
  constexpr int kTile = 2 * kTM * 4;                // 16-byte slots of one step's activation tile: [hi, lo][row][4 k groups]
  static_assert(U % AD == 0 && AD >= 2, "the fragment ring must divide the unroll");
  __shared__ __attribute__((aligned(16))) u32x4 xq[2 * S * kTile];
  __shared__ int rowtab[kMaxSeg * kTM];
  __shared__ unsigned s_mask;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = xcd_contiguous_block() * kTM;
  const int nkc = p.KP / kKC;

  if (tid == 0) s_mask = 0;
  __syncthreads();
  {
    unsigned mine = 0;
    for (int e = tid; e < p.n_seg * kTM; e += NT) {
      const int sg = e / kTM, row = e % kTM;
      const int v = source_row(p, sg, m0 + row);      // every segment has a row map here (the kernel choice)
      rowtab[e] = v;
      mine |= (v >= 0 ? 1u : 0u) << sg;
    }
    if (mine) atomicOr(&s_mask, mine);
  }
  __syncthreads();
  const unsigned act = (unsigned)__builtin_amdgcn_readfirstlane((int)s_mask);
  const int n_steps = __builtin_popcount(act) * nkc;
  const int n_rounds = (n_steps + S - 1) / S, n_iter = (n_rounds + U - 1) / U * U;
  const float* const src = p.seg[0].src;
  const int ld = p.seg[0].ld;

  if (wave >= 4) {
    // ---- loader waves ---------------------------------------------------------------------------------------------------------
    const int ltid = tid - 256, srow = ltid >> 3, sc4 = (ltid & 7) * 4;
    f32x4 xr[U][S][NPASS];
    unsigned vm[U];
    StepIter it = {act, 0};
    auto issue = [&](f32x4 (&x)[S][NPASS], unsigned& valid) __attribute__((always_inline)) {
      valid = 0;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        int sg, kc;
        const bool live = it.next(nkc, sg, kc);
        const int col = kc * kKC + sc4;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
          const int row = srow + RPP * i;
          const int r = row < kTM ? rowtab[sg * kTM + row] : -1;
          const bool ok = live && r >= 0 && col < p.K;
          valid |= (ok ? 1u : 0u) << (j * NPASS + i);
          const unsigned ofs = (unsigned)(r < 0 ? 0 : r) * (unsigned)ld + (unsigned)(col < p.K ? col : 0);
#if V3D_PIPE_ABLATE == 3
          x[j][i] = (f32x4){(float)ofs, 0.f, 0.f, 0.f};
#else
          x[j][i] = *reinterpret_cast<const f32x4*>(src + ofs);
#endif
        }
      }
    };
    auto commit = [&](int slot, const f32x4 (&x)[S][NPASS], unsigned valid) __attribute__((always_inline)) {
#if V3D_PIPE_ABLATE == 4
#pragma unroll
      for (int j = 0; j < S; ++j)
#pragma unroll
        for (int i = 0; i < NPASS; ++i) asm volatile("" ::"v"(x[j][i]));
      return;
#endif
#pragma unroll
      for (int j = 0; j < S; ++j) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
          const int row = srow + RPP * i;
          if (kTM % RPP == 0 || row < kTM) {
            f32x4 v = x[j][i];
            const unsigned keep = 0u - ((valid >> (j * NPASS + i)) & 1u);      // zero row: absent neighbour / behind the end
            v.x = __uint_as_float(__float_as_uint(v.x) & keep); v.y = __uint_as_float(__float_as_uint(v.y) & keep);
            v.z = __uint_as_float(__float_as_uint(v.z) & keep); v.w = __uint_as_float(__float_as_uint(v.w) & keep);
            commit_split(xq + (slot * S + j) * kTile, kTM, row, sc4, v, p.relu_in);
          }
        }
      }
    };
    PHASE_DECL;
#pragma unroll
    for (int u = 0; u < U; ++u) issue(xr[u], vm[u]);
    commit(0, xr[0], vm[0]);
    issue(xr[0], vm[0]);
    __syncthreads();
    PHASE_MARK(7);
#pragma unroll 1
    for (int r0 = 0; r0 < n_iter; r0 += U) {
#pragma unroll
      for (int i = 0; i < U; ++i) {
        commit((i + 1) & 1, xr[(i + 1) % U], vm[(i + 1) % U]);       // round r + 1 -> the slot the matrix waves left a round ago
        PHASE_MARK(4);
        issue(xr[(i + 1) % U], vm[(i + 1) % U]);                     // round r + 1 + U
        PHASE_MARK(5);
        __syncthreads();
        PHASE_MARK(6);
      }
    }
#ifdef V3D_PHASE_TIMING
    if (threadIdx.x == 256 && blockIdx.x < kPhaseSlots)
      for (int i_ = 4; i_ < 8; ++i_) g_phase[blockIdx.x * 8 + i_] = (unsigned long long)ph_acc[i_];
#endif
    return;
  }

  // ---- matrix waves ---------------------------------------------------------------------------------------------------------------
  const int kq = lane >> 4, jn = lane & 15;
  f32x4 acc[NB][MBW];
  zero_acc(acc);
  u32x4 afr[AD][S][2 * MBW];
  StepIter ita = {act, 0};
  const u32x4* const wbase = fragment_base<MBW>(p.wp, wave, lane);
  auto issue_a = [&](u32x4 (&a)[S][2 * MBW]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      int sg, kc;
      ita.next(nkc, sg, kc);
#if V3D_PIPE_ABLATE == 2
#pragma unroll
      for (int m = 0; m < 2 * MBW; ++m) a[j][m] = (u32x4){(unsigned)(size_t)wbase + (unsigned)(sg * nkc + kc), 1u, 2u, 3u};
#else
      load_fragments<MBW>(wbase, sg, kc, nkc, a[j]);
#endif
    }
  };
  PHASE_DECL;
#pragma unroll
  for (int u = 0; u < AD - 1; ++u) issue_a(afr[u]);
  __syncthreads();
  PHASE_MARK(0);
#pragma unroll 1
  for (int r0 = 0; r0 < n_iter; r0 += U) {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int r = r0 + i;
      issue_a(afr[(i + AD - 1) % AD]);                               // round r + AD - 1
      PHASE_MARK(1);
#pragma unroll
      for (int j = 0; j < S; ++j) {
        if (r * S + j < n_steps) {
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            bf16x8 b_hi, b_lo;
            read_b(xq + ((i & 1) * S + j) * kTile, kTM, nb * 16 + jn, kq, b_hi, b_lo);
#pragma unroll
            for (int m = 0; m < MBW; ++m) {
              const bf16x8 a_hi = __builtin_bit_cast(bf16x8, afr[i % AD][j][m]), a_lo = __builtin_bit_cast(bf16x8, afr[i % AD][j][MBW + m]);
#if V3D_PIPE_ABLATE == 1
              asm volatile("" ::"v"(a_hi), "v"(a_lo), "v"(b_hi), "v"(b_lo));
#else
              mfma_split3(a_hi, a_lo, b_hi, b_lo, acc[nb][m]);
#endif
            }
          }
        }
      }
      PHASE_MARK(2);
      __syncthreads();
      PHASE_MARK(3);
    }
  }
  gemm_epilogue<MBW, NB>(p, acc, m0, wave, kq, jn);
#ifdef V3D_PHASE_TIMING
  if (threadIdx.x == 0 && blockIdx.x < kPhaseSlots)
    for (int i_ = 0; i_ < 4; ++i_) g_phase[blockIdx.x * 8 + i_] = (unsigned long long)ph_acc[i_];
#endif
}

}  // namespace

int v3d::launch_rounds(const GemmParams& p, int MBW, int nb, unsigned blocks, hipStream_t s) {
  GemmKernel k = nb != 2 ? nullptr : MBW == 2 ? gemm_gather_rounds_kernel<2, 2, 4> : MBW == 1 ? gemm_gather_rounds_kernel<1, 2, 4> : nullptr;
  return launch_gemm(k, "gemm_gather_rounds_kernel", p, blocks, 256, s);
}

int v3d::launch_pipe(const GemmParams& p, int MBW, int nb, int loaders, int min_blocks, unsigned blocks, hipStream_t s) {
  GemmKernel k = nullptr;
  if (nb == 4 && loaders == 8 && min_blocks == 1) k = MBW == 2 ? gemm_gather_pipe_kernel<2, 4, 8, 1> : MBW == 1 ? gemm_gather_pipe_kernel<1, 4, 8, 1> : nullptr;
  if (nb == 2 && loaders == 4 && min_blocks == 2) k = MBW == 2 ? gemm_gather_pipe_kernel<2, 2, 4, 2> : MBW == 1 ? gemm_gather_pipe_kernel<1, 2, 4, 2> : nullptr;
  return launch_gemm(k, "gemm_gather_pipe_kernel", p, blocks, 256 + 64 * loaders, s);      // the four matrix waves + the loader waves
}
