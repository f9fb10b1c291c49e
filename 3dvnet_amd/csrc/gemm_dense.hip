// The one-step gather-GEMM kernel (gemm_gather.hip is the map of the family, gemm_kernels.h what its kernels share): PointNet's
// large layers, the exact-fp32 path of every caller, and the fallback for sources that are not 16-byte loadable.
#include "gemm_kernels.h"
#include "phase_timing.h"

PHASE_TIMING_UNIT(v3d_debug_gemm_phase_read)

using namespace v3d;

namespace {

// MBW: channel blocks (16 outputs) per wave (N <= 64 * MBW); NB: 16-row blocks per workgroup tile
// (tile = 16 * NB rows: 128 for large problems, 32 when M is small so that more workgroups than CUs
// exist and gather latency is hidden by occupancy).
// BF16: split-bf16 operands or exact fp32; either way the weight slab of a (segment, K chunk) step is staged through LDS, one
// step per pair of barriers.  Segments whose row map is empty for the whole tile are skipped (structured sparsity).
template <int MBW, int NB, bool BF16>
__global__ __launch_bounds__(256) void gemm_gather_kernel(GemmParams p) {
  constexpr int kTM = 16 * NB;
  constexpr int NPASS = (kTM + 31) / 32;      // staging passes of 32 rows
  __shared__ __attribute__((aligned(16))) float xs[kTM * kXS];
  __shared__ __attribute__((aligned(16))) float ws[4 * MBW * 16 * kKC];
  __shared__ int s_act[kMaxSeg], s_list[kMaxSeg], s_nact;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const int m0 = blockIdx.x * kTM;
  const int MB = 4 * MBW;

  f32x4 acc[NB][MBW];
  zero_acc(acc);

  // staging role: 8 lanes x float4 cover the 32 columns of one row; 32 rows per pass
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int nkc = p.KP / kKC;
  constexpr int kWslab = 4 * MBW * 16 * kKC;       // packed floats per (segment, K chunk)
  constexpr int WPT = kWslab / 4 / 256;            // float4 of the weight slab per thread
  static_assert(kWslab % 1024 == 0, "weight slab must split evenly over the workgroup");

  // row source of this thread's staging rows for segment s (-1 = zero row)
  auto rows_of = [&](int s, int (&r)[NPASS]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) r[i] = srow + 32 * i < kTM ? source_row(p, s, m0 + srow + 32 * i) : -1;
  };

  // ---- which segments does this tile need at all? (structured sparsity of the neighbour tables) ---------
  if (tid < kMaxSeg) s_act[tid] = 0;
  __syncthreads();
  for (int s = 0; s < p.n_seg; ++s) {
    bool any = p.seg[s].idx == nullptr;            // identity / conv1d maps are always needed
    if (!any) {
      int r[NPASS];
      rows_of(s, r);
#pragma unroll
      for (int i = 0; i < NPASS; ++i) any |= r[i] >= 0;
    }
    if (any) s_act[s] = 1;                         // benign race: everybody writes the same value
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int s = 0; s < p.n_seg; ++s) if (s_act[s]) s_list[n++] = s;
    s_nact = n;
  }
  __syncthreads();
  const int nact = s_nact;

  // ---- software pipeline over the flat (active segment, K chunk) sequence: the next chunk's gathered rows
  // and weight slab are loaded into registers right after the barrier and land during the MFMA loop -------
  f32x4 xr[NPASS], wr[WPT];     // native vector type: keeps the staging registers out of scratch
  auto issue = [&](int s, int kc, const int (&r)[NPASS]) __attribute__((always_inline)) {
    const Seg sg = p.seg[s];
    const bool vec_ok = (sg.ld % 4 == 0) && (p.K % 4 == 0) && ((reinterpret_cast<size_t>(sg.src) & 15) == 0);
    const int col = kc * kKC + sc4;
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (r[i] >= 0 && col < p.K) {
        const float* rowp = sg.src + (size_t)r[i] * sg.ld + col;
        if (vec_ok) {
          v = *reinterpret_cast<const f32x4*>(rowp);
        } else {
          v.x = rowp[0];
          if (col + 1 < p.K) v.y = rowp[1];
          if (col + 2 < p.K) v.z = rowp[2];
          if (col + 3 < p.K) v.w = rowp[3];
        }
      }
      xr[i] = v;
    }
    const f32x4* wsrc = reinterpret_cast<const f32x4*>(p.wp + (size_t)(s * nkc + kc) * kWslab) + tid;
#pragma unroll
    for (int i = 0; i < WPT; ++i) wr[i] = wsrc[i * 256];
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      if (srow + 32 * i < kTM) {
        const int row = srow + 32 * i;
        if constexpr (BF16) {
          commit_split(reinterpret_cast<u32x4*>(xs), kTM, row, sc4, xr[i], p.relu_in);
        } else {
          f32x4 v = xr[i];
          if (p.relu_in) relu4(v);
          float* d = xs + row * kXS + sc4;
          *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
          *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) reinterpret_cast<f32x4*>(ws)[tid + i * 256] = wr[i];
  };

  PHASE_DECL;
  int rcur[NPASS], rnxt[NPASS];
  if (nact > 0) {
    rows_of(s_list[0], rcur);
    issue(s_list[0], 0, rcur);
    if (nact > 1) rows_of(s_list[1], rnxt);
  }
  PHASE_MARK(0);
  for (int a = 0; a < nact; ++a) {
    for (int kc = 0; kc < nkc; ++kc) {
      __syncthreads();
      PHASE_MARK(1);
      commit();
      PHASE_MARK(2);
      __syncthreads();
      PHASE_MARK(3);
      if (kc + 1 < nkc) {
        issue(s_list[a], kc + 1, rcur);
      } else if (a + 1 < nact) {
#pragma unroll
        for (int i = 0; i < NPASS; ++i) rcur[i] = rnxt[i];
        issue(s_list[a + 1], 0, rcur);
        if (a + 2 < nact) rows_of(s_list[a + 2], rnxt);       // one whole segment ahead of its first use
      }
      PHASE_MARK(4);
      // ---- MFMA ------------------------------------------------------------------------------------------
      if constexpr (BF16) {
        const u32x4* wq = reinterpret_cast<const u32x4*>(ws);
        bf16x8 a_hi[MBW], a_lo[MBW];
#pragma unroll
        for (int m = 0; m < MBW; ++m) {
          a_hi[m] = __builtin_bit_cast(bf16x8, wq[(wave * MBW + m) * 64 + lane]);
          a_lo[m] = __builtin_bit_cast(bf16x8, wq[(MB + wave * MBW + m) * 64 + lane]);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          bf16x8 b_hi, b_lo;
          read_b(reinterpret_cast<const u32x4*>(xs), kTM, nb * 16 + jn, kq, b_hi, b_lo);
#pragma unroll
          for (int m = 0; m < MBW; ++m) mfma_split3(a_hi[m], a_lo[m], b_hi, b_lo, acc[nb][m]);
        }
      } else {
#pragma unroll
        for (int k4 = 0; k4 < kKC / 4; ++k4) {
          float a_frag[MBW];
#pragma unroll
          for (int m = 0; m < MBW; ++m) a_frag[m] = ws[((k4 * MB + wave * MBW + m) * 64) + lane];
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const float bv = xs[(nb * 16 + jn) * kXS + k4 * 4 + kq];
#pragma unroll
            for (int m = 0; m < MBW; ++m)
              acc[nb][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_frag[m], bv, acc[nb][m], 0, 0, 0);
          }
        }
      }
    }
  }

  PHASE_MARK(5);
  gemm_epilogue<MBW, NB>(p, acc, m0, wave, kq, jn);
  PHASE_MARK(6);
  PHASE_FLUSH;
}

}  // namespace

int v3d::launch_dense(const GemmParams& p, int MBW, int nb, bool bf16, unsigned blocks, hipStream_t s) {
  GemmKernel k = nullptr;
  if (MBW == 2 && nb == 2) k = bf16 ? gemm_gather_kernel<2, 2, true> : gemm_gather_kernel<2, 2, false>;
  if (MBW == 2 && nb == 8) k = bf16 ? gemm_gather_kernel<2, 8, true> : gemm_gather_kernel<2, 8, false>;
  if (MBW == 1 && nb == 2) k = bf16 ? gemm_gather_kernel<1, 2, true> : gemm_gather_kernel<1, 2, false>;
  if (MBW == 1 && nb == 8) k = bf16 ? gemm_gather_kernel<1, 8, true> : gemm_gather_kernel<1, 8, false>;
  return launch_gemm(k, "gemm_gather_kernel", p, blocks, 256, s);
}
