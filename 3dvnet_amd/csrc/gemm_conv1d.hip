// The hypothesis decoder's conv1d kernel (gemm_gather.hip is the map of the family, gemm_kernels.h what its kernels share).
#include "gemm_kernels.h"

using namespace v3d;

namespace {

// ---- Conv1d(k = 3, pad 1) over groups of `group_len` consecutive rows (the hypothesis decoder, refinement.py:29-30) ----
// The three taps read the same activation rows shifted by -1 / 0 / +1, so the tile (+ one halo row on either side) is
// gathered, split and committed to LDS once per K chunk and used by all three taps; only the 16 KB weight slab changes
// between taps.  A tap that would cross a group boundary reads a zero row instead (the conv's padding).  The generic
// kernel stages every (tap, chunk) separately: three times the gather + split work, which is the larger half of its time.
template <int MBW, int NB>
__global__ __launch_bounds__(256) void conv1d_gemm_kernel(GemmParams p) {
  constexpr int kTM = 16 * NB, kZRow = kTM + 2, kRT = kTM + 3;      // rows in LDS: halo + tile + halo + zero row
  constexpr int NPASS = (kTM + 2 + 31) / 32;
  __shared__ __attribute__((aligned(16))) u32x4 xq[2 * kRT * 4];     // [hi, lo][row][4 k groups of 8 bf16]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const int m0 = blockIdx.x * kTM;
  const int nkc = p.KP / kKC;
  const float* const src = p.seg[0].src;
  const int ld = p.seg[0].ld;

  f32x4 acc[NB][MBW];
  zero_acc(acc);
  // per column block: does tap 0 / tap 2 of this lane's output row stay inside its group?  (bit 2 nb / 2 nb + 1; a tap
  // that leaves the group reads the zero row = the conv's padding)
  unsigned tapmask = 0;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int hh = (m0 + nb * 16 + jn) % p.group_len;
    tapmask |= (hh >= 1 ? 1u : 0u) << (2 * nb);
    tapmask |= (hh + 1 < p.group_len ? 1u : 0u) << (2 * nb + 1);
  }
  if (tid < 8) xq[(tid >> 2) * kRT * 4 + kZRow * 4 + (tid & 3)] = (u32x4){0u, 0u, 0u, 0u};

  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  f32x4 xr[NPASS];
  auto issue_x = [&](int kc) __attribute__((always_inline)) {
    const int col = kc * kKC + sc4;
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int lr = srow + 32 * i, m = m0 - 1 + lr;
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (lr < kTM + 2 && m >= 0 && m < p.M && col < p.K) v = *reinterpret_cast<const f32x4*>(src + (size_t)m * ld + col);
      xr[i] = v;
    }
  };
  auto commit_x = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int row = srow + 32 * i;
      if (row < kTM + 2) commit_split(xq, kRT, row, sc4, xr[i], p.relu_in);
    }
  };
  // A fragments: every wave owns its MBW channel blocks, nothing is shared between waves, so the fragments go from the
  // packed image (L2-resident) straight into registers, one tap ahead -- no LDS copy, no barrier between taps
  u32x4 a_cur[2 * MBW], a_nxt[2 * MBW];
  const u32x4* const wbase = fragment_base<MBW>(p.wp, wave, lane);

  issue_x(0);
  load_fragments<MBW>(wbase, 0, 0, nkc, a_cur);
#pragma unroll 1
  for (int kc = 0; kc < nkc; ++kc) {
    __syncthreads();                 // the previous chunk's MFMAs are done with the tile
    commit_x();
    __syncthreads();
    if (kc + 1 < nkc) issue_x(kc + 1);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      if (t < 2) load_fragments<MBW>(wbase, t + 1, kc, nkc, a_nxt);
      else if (kc + 1 < nkc) load_fragments<MBW>(wbase, 0, kc + 1, nkc, a_nxt);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const bool inside = t == 1 || ((tapmask >> (2 * nb + (t >> 1))) & 1u);
        bf16x8 b_hi, b_lo;
        read_b(xq, kRT, inside ? nb * 16 + jn + t : kZRow, kq, b_hi, b_lo);
#pragma unroll
        for (int m = 0; m < MBW; ++m)
          mfma_split3(__builtin_bit_cast(bf16x8, a_cur[m]), __builtin_bit_cast(bf16x8, a_cur[MBW + m]), b_hi, b_lo, acc[nb][m]);
      }
#pragma unroll
      for (int m = 0; m < 2 * MBW; ++m) a_cur[m] = a_nxt[m];
    }
  }
  gemm_epilogue<MBW, NB>(p, acc, m0, wave, kq, jn);
}

}  // namespace

int v3d::launch_conv1d(const GemmParams& p, int MBW, int nb, unsigned blocks, hipStream_t s) {
  GemmKernel k = nullptr;
  if (MBW == 2) k = nb == 2 ? conv1d_gemm_kernel<2, 2> : nb == 4 ? conv1d_gemm_kernel<2, 4> : nullptr;
  if (MBW == 1) k = nb == 2 ? conv1d_gemm_kernel<1, 2> : nb == 8 ? conv1d_gemm_kernel<1, 8> : nullptr;
  return launch_gemm(k, "conv1d_gemm_kernel", p, blocks, 256, s);
}
