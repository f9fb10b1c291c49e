// Gather-GEMM on the matrix cores: the dense-arithmetic workhorse of rows B4 (PointNet), B6 (sparse 3D U-Net) and C2b
// (hypothesis decoder conv1d) of SURVEY.md §8a.
//
//   Y[m, :] = epilogue( sum_{s < n_seg}  act(X_s[row_s(m), 0:K]) @ W_s  + bias )
//
// A "segment" is (source matrix, row map, weight slab):
//   * PointNet fcK(relu(cat(x, pool[idx])))  -> 2 segments: (x, identity), (pool, idx)
//                                                (scenemodeling.py:129-141)
//   * sparse conv, 27 kernel offsets           -> 27 segments over one source, row map = column k of
//                                                the neighbour table, -1 = absent voxel = zero row
//                                                (MinkowskiConvolution, scenemodeling.py:36-38,160,181)
//   * conv1d(k3, pad 1) along the 7 hypotheses -> 3 segments, row map m + (s - 1) inside each group
//                                                of `group_len` rows (refinement.py:8-25)
// Epilogue (all optional): + bias, GroupNorm(rows), + residual, ReLU, scatter-max into pool[idx[m]], row-major store.
//
// This file is the host side -- the weight packer, argument validation, the choice of the kernel, the extern "C" entry points --
// and the map of the kernels, one family per translation unit (gemm_kernels.h: the LDS and packed-image layouts, what the
// kernels share -- split-bf16 product, tile staging, row map, fragment load, epilogues -- and their launchers):
//   gemm_dense.hip     gemm_gather_kernel, one (segment, K chunk) step per pair of barriers, weight slab through LDS: large M
//                      (PointNet's 200 k-row layers, 128-row tiles), exact fp32, and whatever the others refuse (sources that
//                      are not 16-byte loadable, K % 4 != 0)
//   gemm_sparse.hip    small M, the sparse convolutions: gemm_gather_rounds_kernel (four steps per pair of barriers, weight
//                      fragments straight into registers) and gemm_gather_pipe_kernel (loader waves + matrix waves, one
//                      barrier per round; the default for a convolution with a neighbour table)
//   gemm_conv1d.hip    conv1d_gemm_kernel: the three taps of the hypothesis decoder's conv1d share one staged tile per K chunk
//   gemm_wgrad.hip     sparse_conv_wgrad_kernel: the weight gradient of a sparse convolution (training): the contraction runs over the
//                      ROWS of a neighbour-table column, exact fp32, partial tiles per row chunk; its own entry point and host side
// The four forward kernels take the steps and multiply in the same order per accumulator and share the epilogue: where more than one
// serves a call their outputs agree bit for bit (tests/test_parity_net_gpu.py).
#include <cstdlib>
#include <vector>

#include "gemm_kernels.h"
#include "gemm_weights.h"
#include "weight_pack.h"

using namespace v3d;

namespace {

// ---- which kernel serves a call ---------------------------------------------------------------------------------------------
enum class GemmKind { conv1d, pipe, rounds, one_step };
struct GemmChoice {
  GemmKind kind;
  int nb;                    // 16-row blocks per tile
  int loaders, min_blocks;   // pipe: loader waves, workgroups per CU the kernel is compiled for
  int tile_rows;             // 16 nb
};

// vec_ok: every segment's source is 16-byte loadable (16-byte aligned, row stride a multiple of 4 floats); one_src: every
// segment reads the same matrix with the same stride; n_maps: segments with a row map; ld0: that stride, in floats.
GemmChoice choose_gemm_kernel(int n_seg, int K, int KP, int MBW, int M, int group_len, int precision, int opt_rounds, int opt_pipe,
                              bool vec_ok, bool one_src, int n_maps, int ld0) {
  const bool small = M < 128 * 1024;           // fewer than ~4 tiles of 128 rows per CU: use 32-row tiles
  const bool fp32_path = precision == V3D_PRECISION_FP32;    // exact-fp32 MFMA instead of split bf16
  const int n_steps = n_seg * (KP / kKC);
  auto choice = [](GemmKind kind, int nb, int loaders, int min_blocks) { return GemmChoice{kind, nb, loaders, min_blocks, 16 * nb}; };
  // conv1d over row groups (3 taps of the same source): the tile is staged once per K chunk for all three taps
  if (!fp32_path && group_len > 0 && n_seg == 3 && K % 4 == 0 && one_src && n_maps == 0 && vec_ok) {
    // one kernel family for every M (32-row tiles when M is small): chunked and unchunked calls of the decoder then
    // accumulate in the same order and agree bit for bit
    // 64-row tiles for large M: 32 accumulator registers instead of 64 -> 4 waves per SIMD (14.3 ms against 16.0 ms with
    // 128-row tiles and 17.9 ms with 32-row tiles on the cfg3 decoder)
    return choice(GemmKind::conv1d, small ? 2 : MBW == 2 ? 4 : 8, 0, 0);
  }
  // small M, split-bf16, every segment 16-byte loadable: the rounds kernel (four steps per pair of barriers)
  const bool rounds = small && !fp32_path && K % 4 == 0 && n_steps >= 2 && KP / kKC <= 8 && opt_rounds != 0 && vec_ok;
  // a sparse convolution (one source, a row map per offset): the loader / matrix pipeline
  const bool pipe = rounds && group_len == 0 && n_steps >= 8 && (size_t)M * (size_t)ld0 < ((size_t)1 << 31) && opt_pipe != 0 &&
                    n_maps == n_seg && one_src;
  if (pipe) {
    // rows per tile: a tile streams the whole weight image through its CU's vector-memory path (27 x K x N x 4 bytes), so
    // the tile is as tall as the number of workgroups allows -- about one per CU on the 128-channel levels, two on the wide
    // 64-channel level
    // measured on the cfg3 scene's levels (rounds kernel -> here): 13 434 rows x 128 channels 84 -> 60 us with 64-row tiles and
    // 8 loader waves, 2 719 x 128: 58 -> 40 us with 32-row tiles and 4 loader waves, 59 975 x 64: 90 -> 84 us
    const bool tall = M >= 8192;
    return tall ? choice(GemmKind::pipe, 4, 8, 1) : choice(GemmKind::pipe, 2, 4, 2);
  }
  // 32-row tiles: a tile re-reads the whole weight image, so L2 -> CU weight traffic is M / 32 x 27 x K x N x 4 bytes
  if (rounds) return choice(GemmKind::rounds, 2, 0, 0);
  return choice(GemmKind::one_step, small ? 2 : 8, 0, 0);
}

__global__ void fill_kernel(float* p, size_t n, float v) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

// ---- packed weights -------------------------------------------------------------------------------

extern "C" int v3d_gemm_pack(const float* w_host, long long stride_seg, long long stride_co,
                             long long stride_k, int n_seg, int N, int K, const float* scale_host,
                             const float* bias_host, const float* gn_w_host, const float* gn_b_host,
                             v3d_gemm_weights** out_handle) {
  V3D_REQUIRE(w_host && out_handle, V3D_ERR_BAD_ARG, "v3d_gemm_pack: null argument");
  V3D_REQUIRE(n_seg >= 1 && n_seg <= kMaxSeg && N >= 1 && N <= 128 && K >= 1, V3D_ERR_BAD_SHAPE,
              "v3d_gemm_pack: unsupported shape (n_seg=%d N=%d K=%d)", n_seg, N, K);
  v3d_gemm_weights* h = new v3d_gemm_weights();
  h->N = N; h->K = K; h->n_seg = n_seg;
  h->KP = (K + kKC - 1) / kKC * kKC;
  h->MBW = N > 64 ? 2 : 1;
  const int MB = 4 * h->MBW, nkc = h->KP / kKC;
  const size_t wslab = (size_t)MB * 16 * kKC;
  std::vector<float> host((size_t)n_seg * nkc * wslab + 3 * 128, 0.f);   // grown below for the bf16 image
  // weight (segment s, output co, k) with the per-output scale folded; 0 in the padding of N and K
  auto weight = [&](int s, int co, int k) {
    float v = 0.f;
    if (co < N && k < K) {
      v = w_host[s * stride_seg + co * stride_co + k * stride_k];
      if (scale_host) v *= scale_host[co];
    }
    return v;
  };
  for (int s = 0; s < n_seg; ++s)
    for (int kc = 0; kc < nkc; ++kc)
      for (int k4 = 0; k4 < kKC / 4; ++k4)
        for (int mb = 0; mb < MB; ++mb)
          for (int lane = 0; lane < 64; ++lane)
            host[((size_t)(s * nkc + kc) * wslab) + ((size_t)(k4 * MB + mb) * 64) + lane] =
                weight(s, mb * 16 + (lane & 15), kc * kKC + k4 * 4 + (lane >> 4));
  h->bias_ofs = (size_t)n_seg * nkc * wslab;
  h->gnw_ofs = h->bias_ofs + 128;
  h->gnb_ofs = h->gnw_ofs + 128;
  // split-bf16 image: per (segment, chunk): [hi, lo][MB][64 lanes][4 words]; lane l holds output co = mb*16 + (l & 15),
  // k = chunk*32 + 8*(l >> 4) + e (e = 0..7, two bf16 per word)
  h->bf_ofs = h->gnb_ofs + 128;
  host.resize(h->bf_ofs + (size_t)n_seg * nkc * wslab, 0.f);
  {
    unsigned* wb = reinterpret_cast<unsigned*>(host.data() + h->bf_ofs);
    for (int s = 0; s < n_seg; ++s)
      for (int kc = 0; kc < nkc; ++kc)
        for (int mb = 0; mb < MB; ++mb)
          for (int lane = 0; lane < 64; ++lane) {
            float v[8];
            for (int e = 0; e < 8; ++e) v[e] = weight(s, mb * 16 + (lane & 15), kc * kKC + 8 * (lane >> 4) + e);
            unsigned* dst = wb + (size_t)(s * nkc + kc) * wslab + ((size_t)mb * 64 + lane) * 4;
            split_bf16x8(v, dst, dst + (size_t)MB * 256);
          }
  }
  // the fused hypothesis decoder's image (gemm_weights.h, dec_ofs)
  h->dec_ofs = 0;
  if (n_seg == 3 && N == 128 && K % 16 == 0) {
    const int nst = K / 16;
    h->dec_ofs = host.size();
    host.resize(h->dec_ofs + (size_t)nst * 24 * 256, 0.f);
    unsigned* wb = reinterpret_cast<unsigned*>(host.data() + h->dec_ofs);
    for (int st = 0; st < nst; ++st)
      for (int t = 0; t < 3; ++t)
        for (int mb = 0; mb < 4; ++mb)
          for (int lane = 0; lane < 64; ++lane) {
            const int co = mb * 32 + (lane & 31), g = lane >> 5;
            float v[8];
            for (int e = 0; e < 8; ++e) v[e] = weight(t, co, 16 * st + 8 * (e >> 2) + 4 * g + (e & 3));
            unsigned* dst = wb + ((((size_t)st * 3 + t) * 2) * 4 + mb) * 256 + (size_t)lane * 4;
            split_bf16x8(v, dst, dst + 4 * 256);
          }
  }
  h->has_bias = bias_host != nullptr;
  h->has_gn = gn_w_host != nullptr && gn_b_host != nullptr;
  for (int i = 0; i < N; ++i) {
    if (bias_host) host[h->bias_ofs + i] = bias_host[i];
    if (h->has_gn) { host[h->gnw_ofs + i] = gn_w_host[i]; host[h->gnb_ofs + i] = gn_b_host[i]; }
  }
  return finish_pack(h, host.data(), host.size() * sizeof(float), "gemm weights", out_handle);
}

extern "C" void v3d_gemm_free(v3d_gemm_weights* h) { release(h); }

extern "C" int v3d_gemm_gather_f32(const v3d_gemm_weights* h, int M, const float* const* seg_src_host,
                                   const int32_t* const* seg_idx_host, const int* seg_ld_host,
                                   int group_len, int relu_in, int use_gn, float gn_eps,
                                   const float* residual, int ld_res, int relu_out, float* pool,
                                   const int32_t* pool_idx, int ld_pool, float* out, int ld_out,
                                   int precision, void* stream) {
  V3D_REQUIRE(h && seg_src_host && seg_ld_host, V3D_ERR_BAD_ARG, "v3d_gemm_gather_f32: null argument");
  V3D_REQUIRE(precision == V3D_PRECISION_SPLIT_BF16 || precision == V3D_PRECISION_FP32, V3D_ERR_BAD_ARG,
              "v3d_gemm_gather_f32: unknown precision %d", precision);
  V3D_REQUIRE(M >= 0, V3D_ERR_BAD_SHAPE, "v3d_gemm_gather_f32: M < 0");
  V3D_REQUIRE(use_gn == 0 || use_gn == 1 || use_gn == 8 || use_gn == 16, V3D_ERR_BAD_ARG,
              "v3d_gemm_gather_f32: use_gn = %d (0 off, 1 or 16: 16-channel groups, 8: 8-channel groups)", use_gn);
  V3D_REQUIRE(!use_gn || (h->has_gn && h->N % 16 == 0), V3D_ERR_BAD_ARG,
              "v3d_gemm_gather_f32: GroupNorm requested but weights carry no affine / N %% 16 != 0");
  V3D_REQUIRE(!pool || pool_idx, V3D_ERR_BAD_ARG, "v3d_gemm_gather_f32: pool without pool_idx");
  if (M == 0) return V3D_OK;
  GemmParams p;
  memset(&p, 0, sizeof(p));
  for (int s = 0; s < h->n_seg; ++s) {
    V3D_REQUIRE(seg_src_host[s], V3D_ERR_BAD_ARG, "v3d_gemm_gather_f32: segment %d has no source", s);
    p.seg[s].src = seg_src_host[s];
    p.seg[s].idx = seg_idx_host ? seg_idx_host[s] : nullptr;
    p.seg[s].ld = seg_ld_host[s];
  }
  p.n_seg = h->n_seg; p.M = M; p.N = h->N; p.K = h->K; p.KP = h->KP;
  p.group_len = group_len; p.relu_in = relu_in;
  p.wp = h->dev; p.bias = h->has_bias ? h->dev + h->bias_ofs : nullptr;
  p.gn_w = use_gn ? h->dev + h->gnw_ofs : nullptr; p.gn_b = use_gn ? h->dev + h->gnb_ofs : nullptr;
  p.gn_eps = gn_eps; p.gn8 = use_gn == 8;
  p.residual = residual; p.ld_res = ld_res; p.relu_out = relu_out;
  p.pool = pool; p.pool_idx = pool_idx; p.ld_pool = ld_pool;
  p.out = out; p.ld_out = ld_out;
  hipStream_t s = (hipStream_t)stream;
  if (precision != V3D_PRECISION_FP32) p.wp = h->dev + h->bf_ofs;
  bool vec_ok = true, one_src = true;
  int n_maps = 0;
  for (int t = 0; t < h->n_seg; ++t) {
    vec_ok = vec_ok && p.seg[t].ld % 4 == 0 && (reinterpret_cast<size_t>(p.seg[t].src) & 15) == 0;
    one_src = one_src && p.seg[t].src == p.seg[0].src && p.seg[t].ld == p.seg[0].ld;
    n_maps += p.seg[t].idx != nullptr;
  }
  const GemmChoice c = choose_gemm_kernel(h->n_seg, h->K, h->KP, h->MBW, M, group_len, precision, option(kOptGemmRounds),
                                          option(kOptGemmPipe), vec_ok, one_src, n_maps, p.seg[0].ld);
  const unsigned blocks = (unsigned)((M + c.tile_rows - 1) / c.tile_rows);
  TimedScope ts(h->n_seg == 27 ? "sparse_conv_gemm" : h->n_seg == 3 ? "conv1d_gemm" : "linear_gemm", s);
  switch (c.kind) {
    case GemmKind::conv1d: return launch_conv1d(p, h->MBW, c.nb, blocks, s);
    case GemmKind::pipe: return launch_pipe(p, h->MBW, c.nb, c.loaders, c.min_blocks, blocks, s);
    case GemmKind::rounds: return launch_rounds(p, h->MBW, c.nb, blocks, s);
    default: return launch_dense(p, h->MBW, c.nb, precision != V3D_PRECISION_FP32, blocks, s);
  }
}

extern "C" int v3d_sparse_conv_f32(const v3d_gemm_weights* h, int M, const float* src, int ld_src, const int32_t* nbr,
                                   long long nbr_stride, int use_gn, float gn_eps, const float* residual, int ld_res,
                                   int relu_out, float* out, int ld_out, int precision, void* stream) {
  V3D_REQUIRE(h && src && nbr, V3D_ERR_BAD_ARG, "v3d_sparse_conv_f32: null argument");
  V3D_REQUIRE(nbr_stride >= M, V3D_ERR_BAD_SHAPE, "v3d_sparse_conv_f32: nbr_stride %lld < M %d", nbr_stride, M);
  const float* srcs[kMaxSeg];
  const int32_t* idxs[kMaxSeg];
  int lds[kMaxSeg];
  for (int s = 0; s < h->n_seg; ++s) {
    srcs[s] = src;
    idxs[s] = nbr + (size_t)s * (size_t)nbr_stride;
    lds[s] = ld_src;
  }
  return v3d_gemm_gather_f32(h, M, srcs, idxs, lds, 0, 0, use_gn, gn_eps, residual, ld_res, relu_out, nullptr, nullptr, 0, out,
                             ld_out, precision, stream);
}

extern "C" int v3d_fill_f32(float* ptr, size_t n, float value, void* stream) {
  V3D_REQUIRE(ptr || n == 0, V3D_ERR_BAD_ARG, "v3d_fill_f32: null pointer");
  if (n == 0) return V3D_OK;
  fill_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(ptr, n, value);
  V3D_CHECK_LAUNCH("fill_kernel");
  return V3D_OK;
}

// PointNet input rows (lightningmodel.py:180-183): x[i] = [pts[e1[i]] - anchor_pts[e0[i]] | pts_feat[e1[i]]] in one pass
// (the reference builds it with two index gathers, a subtraction, a third gather and a torch.cat).  4 threads per row.
namespace {
__global__ __launch_bounds__(256) void pointnet_input_kernel(const float* __restrict__ pts, const float* __restrict__ anchor,
                                                             const float* __restrict__ feat, const long long* __restrict__ e0,
                                                             const long long* __restrict__ e1, int n, int C, float* __restrict__ out) {
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i = gid >> 2;
  const int part = (int)(gid & 3);
  if (i >= n) return;
  const long long a = e0[i], q = e1[i];
  float* const o = out + (size_t)i * (3 + C);
  if (part == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = pts[(size_t)q * 3 + d] - anchor[(size_t)a * 3 + d];
  }
  const float* const f = feat + (size_t)q * C;
  for (int c = part; c < C; c += 4) o[3 + c] = f[c];
}
}  // namespace

extern "C" int v3d_pointnet_input_f32(const float* pts, const float* anchor_pts, const float* pts_feat, const int64_t* edge_anchor,
                                      const int64_t* edge_pt, int n_edges, int C, float* out, void* stream) {
  V3D_REQUIRE(pts && anchor_pts && pts_feat && edge_anchor && edge_pt && out, V3D_ERR_BAD_ARG, "v3d_pointnet_input_f32: null argument");
  V3D_REQUIRE(n_edges >= 0 && C >= 1, V3D_ERR_BAD_SHAPE, "v3d_pointnet_input_f32: bad shape");
  if (n_edges == 0) return V3D_OK;
  const long long threads = (long long)n_edges * 4;
  pointnet_input_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      pts, anchor_pts, pts_feat, (const long long*)edge_anchor, (const long long*)edge_pt, n_edges, C, out);
  V3D_CHECK_LAUNCH("pointnet_input_kernel");
  return V3D_OK;
}
