// The weight gradient of a sparse convolution (training): the one member of the gather-GEMM family
// (gemm_gather.hip is its map) that contracts over the ROWS,
//
//   dW[k, ci, co] = sum over the rows p with nbr[k, p] >= 0 of  x[nbr[k, p], ci] * g[p, co]
//
// for the neighbour table `nbr` of the forward.  One workgroup per (row chunk, offset k): it compacts the present rows of its
// chunk, in row order, 512 table entries at a time (developer option "wgrad_compact" = 0: every row, absent ones as zero rows: the
// same terms, measured in DESIGN.md 4.1e), stages 32 of them per tile -- the gathered x rows and the dense g rows, 16-byte
// loads, the ragged tail zero-filled -- and accumulates the K x N tile in registers with the exact-fp32 matrix instruction
// (v_mfma_f32_16x16x4_f32: a weight gradient sums tens of thousands of terms that cancel).  The four waves own the quadrants of
// the tile: at K = N = 128 that is 4 x 4 blocks of 16 x 16, 64 accumulator registers per lane.  The partial tile goes to
// workspace[chunk][k]; a second kernel adds the partials in chunk order and writes every element of grad_w.  No float atomics:
// the bits depend on M, K, N and the inputs only -- the chunking is a function of M alone (wgrad_chunks below is its one
// statement), never of the device.
#include "v3d_common.h"

using namespace v3d;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgradRows = 512;        // table entries per compaction block; a chunk is a whole number of blocks
constexpr int kWgradMaxChunks = 128;   // more than 128 * 512 rows: chunks of 2, 3, ... blocks
constexpr int kWgradTile = 32;         // present rows staged per pair of barriers
constexpr int kWgradLd = 144;          // widest LDS row, lds_stride(128)
constexpr int kWgradMaxRows = 1 << 30; // row indices and chunk ends are int: M + a chunk of rows stays below 2^31

struct WgradChunks { int n, rows; };   // number of chunks, rows per chunk
WgradChunks wgrad_chunks(int M) {
  const int nblk = (M + kWgradRows - 1) / kWgradRows;
  const int per = (nblk + kWgradMaxChunks - 1) / kWgradMaxChunks;
  return {per ? (nblk + per - 1) / per : 0, per * kWgradRows};
}

// Row stride of a staged tile, in floats: = 16 (mod 64), so that the four 16-lane groups of an operand read (rows 4 k4 + 0..3,
// 16 consecutive channels each) fall into disjoint banks.
__host__ __device__ constexpr int lds_stride(int C) { return (C - 16 + 63) / 64 * 64 + 16; }

struct WgradParams {
  const float* src; int ld_src;
  const int* nbr; long long nbr_stride;
  const float* g; int ld_g;
  int M, K, N, n_seg, chunk_rows;
  int compact;                           // developer option "wgrad_compact": 0 = absent rows are staged too, as zero rows
  float* ws;
};

// KBW x NBW: the 16 x 16 blocks a wave owns (wave = 2 wr + wc: ci blocks wr KBW + i, co blocks wc NBW + j).  A block behind K / 16
// or N / 16 recomputes block 0 and stores nothing.
template <int KBW, int NBW>
__global__ __launch_bounds__(256) void sparse_conv_wgrad_kernel(WgradParams p) {
  __shared__ __attribute__((aligned(16))) float xs[kWgradTile * kWgradLd];
  __shared__ __attribute__((aligned(16))) float gs[kWgradTile * kWgradLd];
  __shared__ int plist[kWgradRows], rlist[kWgradRows];   // the present rows of the block, in row order: p and nbr[k, p]
  __shared__ int wcount[2 * 4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kq = lane >> 4, jn = lane & 15;
  const int chunk = blockIdx.x, k = blockIdx.y;
  const int XS = lds_stride(p.K), GS = lds_stride(p.N);
  const int nkb = p.K >> 4, nnb = p.N >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  int acol[KBW], bcol[NBW];
#pragma unroll
  for (int i = 0; i < KBW; ++i) acol[i] = (wr * KBW + i < nkb ? wr * KBW + i : 0) * 16 + jn;
#pragma unroll
  for (int j = 0; j < NBW; ++j) bcol[j] = (wc * NBW + j < nnb ? wc * NBW + j : 0) * 16 + jn;

  f32x4 acc[KBW][NBW];
#pragma unroll
  for (int i = 0; i < KBW; ++i)
#pragma unroll
    for (int j = 0; j < NBW; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int c0 = chunk * p.chunk_rows;
  const int c1 = p.M - c0 < p.chunk_rows ? p.M : c0 + p.chunk_rows;
  const int* const nb = p.nbr + (size_t)k * (size_t)p.nbr_stride;
  // staging role: 32 lanes x 16 bytes cover the 128 columns of a row, 8 rows per pass
  const int srow = tid >> 5, sc = (tid & 31) * 4;
  const bool x_col = sc < p.K, g_col = sc < p.N;

  for (int b0 = c0; b0 < c1; b0 += kWgradRows) {
    __syncthreads();                   // the previous block's tiles are done with the lists
    // ---- the present rows of the block, compacted in row order ------------------------------------------------------------
    int r[2], pre[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = b0 + h * 256 + tid;
      r[h] = e < c1 ? nb[e] : -1;
      const unsigned long long m = __ballot(p.compact ? r[h] >= 0 : e < c1);
      pre[h] = __builtin_popcountll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wcount[h * 4 + wave] = __builtin_popcountll(m);
    }
    __syncthreads();
    int np = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int c = wcount[h * 4 + w];
        if (w == wave && (p.compact ? r[h] >= 0 : b0 + h * 256 + tid < c1)) {
          plist[np + pre[h]] = b0 + h * 256 + tid;
          rlist[np + pre[h]] = r[h];
        }
        np += c;
      }
    }
    __syncthreads();
    const int nt = (np + kWgradTile - 1) / kWgradTile;

    f32x4 xr[4], gr[4];
    auto load = [&](int t) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = t * kWgradTile + srow + 8 * i;
        const int rq = q < np ? rlist[q] : -1;
        const bool ok = rq >= 0;                                  // behind the list, or (wgrad_compact = 0) an absent row
        const int rr = ok ? rq : 0, pp = ok ? plist[q] : 0;
        xr[i] = (ok && x_col) ? *reinterpret_cast<const f32x4*>(p.src + (size_t)rr * (size_t)p.ld_src + sc) : (f32x4){0.f, 0.f, 0.f, 0.f};
        gr[i] = (ok && g_col) ? *reinterpret_cast<const f32x4*>(p.g + (size_t)pp * (size_t)p.ld_g + sc) : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    };
    if (nt > 0) load(0);
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      __syncthreads();                 // the previous tile's matrix instructions have read the LDS tiles
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = srow + 8 * i;
        if (x_col) *reinterpret_cast<f32x4*>(xs + row * XS + sc) = xr[i];
        if (g_col) *reinterpret_cast<f32x4*>(gs + row * GS + sc) = gr[i];
      }
      __syncthreads();
      if (t + 1 < nt) load(t + 1);     // the next tile's loads fly during this tile's matrix instructions
#pragma unroll
      for (int k4 = 0; k4 < kWgradTile / 4; ++k4) {
        float a[KBW], b[NBW];
        // lane l holds A[l & 15][l >> 4] = x[row 4 k4 + (l >> 4)][ci = block + (l & 15)], B[l >> 4][l & 15] likewise from g
#pragma unroll
        for (int i = 0; i < KBW; ++i) a[i] = xs[(k4 * 4 + kq) * XS + acol[i]];
#pragma unroll
        for (int j = 0; j < NBW; ++j) b[j] = gs[(k4 * 4 + kq) * GS + bcol[j]];
#pragma unroll
        for (int i = 0; i < KBW; ++i)
#pragma unroll
          for (int j = 0; j < NBW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
  }

  // ---- the partial tile: accumulator r of a lane is (ci = block + 4 (l >> 4) + r, co = block + (l & 15)) --------------------------
  float* const out = p.ws + ((size_t)chunk * (size_t)p.n_seg + (size_t)k) * (size_t)(p.K * p.N);
#pragma unroll
  for (int i = 0; i < KBW; ++i) {
    const int cib = wr * KBW + i;
    if (cib >= nkb) continue;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      const int cob = wc * NBW + j;
      if (cob >= nnb) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) out[(cib * 16 + kq * 4 + q) * p.N + cob * 16 + jn] = acc[i][j][q];
    }
  }
}

// grad_w = the partial tiles added in chunk order; no chunk at all (M == 0): zeros.
__global__ __launch_bounds__(256) void sparse_conv_wgrad_reduce_kernel(const f32x4* __restrict__ ws, int n_chunks, int slab4,
                                                                       f32x4* __restrict__ grad_w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= slab4) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < n_chunks; ++c) s += ws[(size_t)c * (size_t)slab4 + i];
  grad_w[i] = s;
}

typedef void (*WgradKernel)(WgradParams);
template <int KBW>
WgradKernel wgrad_kernel_n(int nbw) {
  switch (nbw) {
    case 1: return sparse_conv_wgrad_kernel<KBW, 1>;
    case 2: return sparse_conv_wgrad_kernel<KBW, 2>;
    case 3: return sparse_conv_wgrad_kernel<KBW, 3>;
    case 4: return sparse_conv_wgrad_kernel<KBW, 4>;
  }
  return nullptr;
}
WgradKernel wgrad_kernel(int kbw, int nbw) {
  switch (kbw) {
    case 1: return wgrad_kernel_n<1>(nbw);
    case 2: return wgrad_kernel_n<2>(nbw);
    case 3: return wgrad_kernel_n<3>(nbw);
    case 4: return wgrad_kernel_n<4>(nbw);
  }
  return nullptr;
}

bool wgrad_shape_ok(int M, int n_seg, int K, int N) {
  return M >= 0 && M <= kWgradMaxRows && n_seg >= 1 && n_seg <= 27 && K >= 16 && K <= 128 && K % 16 == 0 && N >= 16 && N <= 128 && N % 16 == 0;
}

}  // namespace

extern "C" size_t v3d_sparse_conv_weight_grad_workspace_bytes(int M, int n_seg, int K, int N) {
  if (!wgrad_shape_ok(M, n_seg, K, N)) return 0;
  return (size_t)wgrad_chunks(M).n * (size_t)n_seg * (size_t)(K * N) * sizeof(float);
}

extern "C" int v3d_sparse_conv_weight_grad_f32(const float* src, int ld_src, const int32_t* nbr, long long nbr_stride, int n_seg,
                                               const float* grad_out, int ld_grad, int M, int K, int N, float* grad_w,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(wgrad_shape_ok(M, n_seg, K, N), V3D_ERR_BAD_SHAPE,
              "v3d_sparse_conv_weight_grad_f32: unsupported shape (M=%d n_seg=%d K=%d N=%d): 0 <= M <= 2^30, 1 <= n_seg <= 27, K and N multiples of 16 in [16, 128]",
              M, n_seg, K, N);
  V3D_REQUIRE(ld_src >= K && ld_grad >= N && nbr_stride >= M, V3D_ERR_BAD_SHAPE,
              "v3d_sparse_conv_weight_grad_f32: ld_src %d < K %d, ld_grad %d < N %d or nbr_stride %lld < M %d", ld_src, K, ld_grad, N,
              nbr_stride, M);
  const size_t need = v3d_sparse_conv_weight_grad_workspace_bytes(M, n_seg, K, N);
  V3D_REQUIRE(grad_w && (M == 0 || (src && nbr && grad_out && workspace)), V3D_ERR_BAD_ARG,
              "v3d_sparse_conv_weight_grad_f32: null argument");
  V3D_REQUIRE(workspace_bytes >= need, V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_sparse_conv_weight_grad_f32: workspace %zu < %zu bytes",
              workspace_bytes, need);
  // the staging loads and the partial tiles are 16 bytes wide
  V3D_REQUIRE(ld_src % 4 == 0 && ld_grad % 4 == 0 &&
                  ((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(grad_out) | reinterpret_cast<size_t>(grad_w) |
                    reinterpret_cast<size_t>(workspace)) & 15) == 0,
              V3D_ERR_BAD_ARG, "v3d_sparse_conv_weight_grad_f32: src, grad_out, grad_w and workspace must be 16-byte aligned, ld_src and ld_grad multiples of 4");
  hipStream_t s = (hipStream_t)stream;
  const WgradChunks ch = wgrad_chunks(M);
  TimedScope ts("sparse_conv_wgrad", s);
  if (ch.n > 0) {
    WgradParams p = {src, ld_src, nbr, nbr_stride, grad_out, ld_grad, M, K, N, n_seg, ch.rows, option(kOptWgradCompact) != 0,
                     static_cast<float*>(workspace)};
    WgradKernel kern = wgrad_kernel((K / 16 + 1) / 2, (N / 16 + 1) / 2);
    V3D_REQUIRE(kern, V3D_ERR_BAD_SHAPE, "v3d_sparse_conv_weight_grad_f32: no kernel for K=%d N=%d", K, N);
    kern<<<dim3((unsigned)ch.n, (unsigned)n_seg), 256, 0, s>>>(p);
    V3D_CHECK_LAUNCH("sparse_conv_wgrad_kernel");
  }
  const int slab4 = n_seg * K * N / 4;
  sparse_conv_wgrad_reduce_kernel<<<(unsigned)((slab4 + 255) / 256), 256, 0, s>>>(static_cast<const f32x4*>(workspace), ch.n, slab4,
                                                                                 reinterpret_cast<f32x4*>(grad_w));
  V3D_CHECK_LAUNCH("sparse_conv_wgrad_reduce_kernel");
  return V3D_OK;
}
