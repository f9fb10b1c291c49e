// Sparse trilinear interpolation at arbitrary query points (MinkowskiInterpolation, mv3d/subnetworks/refinement.py:26,39) on the
// hashed levels of sparse.hip, written straight into the decoder's wide feature row; its backward with respect to the features;
// the corner table of the fused hypothesis decoder (decoder.hip).  Both corner kernels state the corner through interp_corner.
#include <optional>

#include "sparse_interp.h"
#include <rocprim/rocprim.hpp>      // after v3d_common.h (<cstring>: rocprim's texture iterator calls the host memset)

namespace {

using namespace v3dhash;
using namespace v3dinterp;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Sparse trilinear interpolation in two kernels:
//  1. corners: one thread per (query, corner) -- the 8 hash probes of a query run in parallel lanes and
//     leave (row, weight) pairs in a small scratch table (row -1 = absent corner, weight unused);
//  2. gather:  C/4 threads per query, float4 channels each; the 8 feature-row loads are independent
//     (no probe in between), so they are all in flight together.
template <bool POW2>
__global__ __launch_bounds__(256) void interp_corners_kernel(Level L, const float* __restrict__ pts, const long long* __restrict__ pts_batch,
                                                             int n_hyp, int n_query, int* __restrict__ crow, float* __restrict__ cw) {
  const int gid = blockIdx.x * 256 + threadIdx.x, q = gid >> 3;
  if (q >= n_query) return;
  const float* p = pts + (size_t)q * 3;
  const Corner c = interp_corner<POW2>(L, (int)pts_batch[q / n_hyp], p[0], p[1], p[2], gid & 7);
  crow[gid] = c.row; cw[gid] = c.w;
}

__global__ __launch_bounds__(256) void interp_gather_kernel(const float* __restrict__ feats, int C,
                                                            const int* __restrict__ crow,
                                                            const float* __restrict__ cw, int n_query,
                                                            float* __restrict__ out, int ld_out, int col0) {
  const int tpq = C / 4;                       // threads per query
  const int q = (blockIdx.x * 256 + threadIdx.x) / tpq;
  const int c4 = ((blockIdx.x * 256 + threadIdx.x) % tpq) * 4;
  if (q >= n_query) return;
  int rows[8];
  float w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { rows[k] = crow[q * 8 + k]; w[k] = cw[q * 8 + k]; }
  float4 f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k)
    f[k] = rows[k] >= 0 ? *reinterpret_cast<const float4*>(feats + (size_t)rows[k] * C + c4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {        // corner order x fastest, as in the single-kernel formulation
    if (rows[k] >= 0) { acc.x += w[k] * f[k].x; acc.y += w[k] * f[k].y; acc.z += w[k] * f[k].z; acc.w += w[k] * f[k].w; }
  }
  float* o = out + (size_t)q * ld_out + col0 + c4;
  o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = acc.w;
}

// ---- the corner table of the fused decoder -----------------------------------------------------------------------------------------
struct CornerParams {
  Level level[3];
  const float* pts;            // [n_q, 3]
  const long long* pts_batch;  // [n_pts]
  int n_hyp;
  unsigned m_hyp;              // v3d::magic_u32 of n_hyp
  int n_q;                     // n_pts * n_hyp
  u32x2* out;                  // [n_q][3 levels][8 corners] (feature row, weight bits); absent corner = (0, 0.f)
};

#ifdef V3D_CORNER_STATS
// developer build only (scripts/micro/corner_stats.py): [level][0 lookups, 1 probes, 2 longest chain, 3 present]
__device__ unsigned long long g_corner_stats[12];
struct CountedFind {
  int l;
  __device__ __forceinline__ int operator()(const HashTable& t, unsigned long long key) const {
    unsigned slot = hash_u64(key) & t.mask;
    int row = -1;
    unsigned probe = 0;
    for (; probe <= t.mask; ++probe) {
      const unsigned long long k = t.entries[slot].key;
      if (k == key) { row = t.entries[slot].val; break; }
      if (k == kEmpty) break;
      slot = (slot + 1) & t.mask;
    }
    atomicAdd(&g_corner_stats[l * 4 + 0], 1ull);
    atomicAdd(&g_corner_stats[l * 4 + 1], (unsigned long long)(probe + 1));
    atomicMax(&g_corner_stats[l * 4 + 2], (unsigned long long)(probe + 1));
    if (row >= 0) atomicAdd(&g_corner_stats[l * 4 + 3], 1ull);
    return row;
  }
};
#endif

// Rows C2a's index half: the 8 lattice corners of every hypothesis point on the three levels.  One thread per (row, corner), the
// three levels in turn.  What bounds the kernel is the number of L2 requests, not the instructions: 34 M random 8-byte key reads +
// 16 M value reads per 64-view sweep in 0.23 ms are ~0.2 T requests/s, the rate of the L2 channels (one thread per (row, level,
// corner) -- a third of the instructions per thread, three times the threads re-reading the point -- measured 0.28 ms against 0.23).
template <bool POW2>
__global__ __launch_bounds__(256) void decoder_corner_kernel(CornerParams cp) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;      // (host: 8 n_q < 2^31)
  const unsigned q = gid >> 3;
  const int corner = (int)(gid & 7u);
  if (q >= (unsigned)cp.n_q) return;
  const int b = (int)cp.pts_batch[v3d::udiv_magic(q, (unsigned)cp.n_hyp, cp.m_hyp)];
  const float px = cp.pts[(size_t)q * 3 + 0], py = cp.pts[(size_t)q * 3 + 1], pz = cp.pts[(size_t)q * 3 + 2];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
#ifdef V3D_CORNER_STATS
    const Corner c = interp_corner<POW2>(cp.level[l], b, px, py, pz, corner, CountedFind{l});
#else
    const Corner c = interp_corner<POW2>(cp.level[l], b, px, py, pz, corner);
#endif
    // an absent corner reads feature row 0 with weight 0: the gathers of the fused kernel are unconditional
    cp.out[((size_t)q * 3 + l) * 8 + corner] = (u32x2){c.row < 0 ? 0u : (unsigned)c.row, c.row < 0 ? 0u : __float_as_uint(c.w)};
  }
}

// ---- backward of the interpolation with respect to feats ------------------------------------------------------------------------
// grad_feats[r] = sum over the corner slots (q, k) with row r of w(q, k) * grad_out[q].  A level of a few thousand rows receives
// n_query * 8 contribution rows: with float atomics every adder would sit on a handful of rows.  Instead the corner slots are
// grouped by row once (v3d_segment_csr: stable, so a row's list is in slot order) and every row's list is summed in list order.
// The contributions are never stored: a slot's contribution is w * grad_out[slot >> 3], read back through the index -- the
// 8 reads per query the forward makes.  A voxel on a wall seen by many views has thousands of slots (on the coarse levels of
// the reference's training shape even the median row has: DESIGN.md 4.1d), so lists are cut into chunks of kInterpBwdChunk slots, each summed by its own lane group (C / 4 lanes x float4); a row of one
// chunk is written straight to grad_feats, the chunks of a longer row to `partial` and added in chunk order by the combine
// kernel.  Every order is fixed by the sort: the result is the same bits from call to call.
constexpr int kInterpBwdChunk = 512;

// absent corners (-1) go to the extra segment n_in, which nobody sums
__global__ __launch_bounds__(256) void interp_backward_segment_kernel(int* __restrict__ crow, int n, int n_in) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;      // unsigned: the last workgroup's indices may pass 2^31
  if (i < (unsigned)n && crow[i] < 0) crow[i] = n_in;
}

// chunks of row r: at least one (a row nobody touches is written as +0 by its single, empty chunk); nch[n_in] = 0 so that the
// exclusive scan over n_in + 1 elements ends in the total
__global__ __launch_bounds__(256) void interp_backward_count_kernel(const int* __restrict__ offsets, int n_in,
                                                                    int* __restrict__ nch) {
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  if (r > (unsigned)n_in) return;
  int c = 0;
  if (r < (unsigned)n_in) {
    const int cnt = offsets[r + 1] - offsets[r];
    c = cnt > kInterpBwdChunk ? (cnt + kInterpBwdChunk - 1) / kInterpBwdChunk : 1;
  }
  nch[r] = c;
}

template <bool VEC>
__device__ __forceinline__ float4 interp_backward_load(const float* p) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// partial slot of chunk j of a row with nch >= 2 chunks: 2 X + j, X = chunk_ofs[r] - r = the chunks beyond the first of all
// earlier rows.  The next such row starts at >= 2 (X + nch - 1) >= 2 X + nch: no overlap, and 2 X + j <= 2 (n / kInterpBwdChunk).
__device__ __forceinline__ size_t interp_backward_slot(int chunk_ofs_r, int r, int j) {
  return 2 * (size_t)(chunk_ofs_r - r) + (size_t)j;
}

// C / 4 lanes per chunk, 256 / (C / 4) chunks per workgroup.  The grid covers the static bound n / kInterpBwdChunk + n_in; the
// chunks that exist are [0, chunk_ofs[n_in]).  VEC: grad_out rows can be read 16 bytes at a time.
template <bool VEC>
__global__ __launch_bounds__(256) void interp_backward_chunk_kernel(const int* __restrict__ perm, const int* __restrict__ offsets,
                                                                    const int* __restrict__ chunk_ofs, int n_in, int C,
                                                                    const float* __restrict__ cw,
                                                                    const float* __restrict__ grad_out, int ld_grad, int col0,
                                                                    float* __restrict__ grad_feats, float* __restrict__ partial) {
  const int tpc = C / 4, sh = __builtin_ctz(tpc);         // 256 % tpc == 0: a power of two
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int chunk = (int)(gid >> sh), c4 = (int)(gid & (tpc - 1)) * 4;
  if (chunk >= chunk_ofs[n_in]) return;
  int lo = 0, hi = n_in;                          // the row r with chunk_ofs[r] <= chunk < chunk_ofs[r + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_ofs[mid] <= chunk) lo = mid; else hi = mid;
  }
  const int r = lo, first = chunk_ofs[r], j = chunk - first, nch = chunk_ofs[r + 1] - first;
  const int b = offsets[r] + j * kInterpBwdChunk, end = offsets[r + 1];      // b + chunk may pass 2^31: compare differences
  const int e = end - b > kInterpBwdChunk ? b + kInterpBwdChunk : end;
  const float* g0 = grad_out + col0 + c4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int i = b;
  for (; e - i >= 8; i += 8) {                    // 8 independent (slot -> weight, gradient row) chains in flight, summed in list order
    int slot[8];
    float w[8];
    float4 g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) slot[k] = perm[i + k];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      w[k] = cw[slot[k]];
      g[k] = interp_backward_load<VEC>(g0 + (size_t)(slot[k] >> 3) * ld_grad);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { acc.x += w[k] * g[k].x; acc.y += w[k] * g[k].y; acc.z += w[k] * g[k].z; acc.w += w[k] * g[k].w; }
  }
  for (; i < e; ++i) {
    const int slot = perm[i];
    const float w = cw[slot];
    const float4 g = interp_backward_load<VEC>(g0 + (size_t)(slot >> 3) * ld_grad);
    acc.x += w * g.x; acc.y += w * g.y; acc.z += w * g.z; acc.w += w * g.w;
  }
  float* dst = nch == 1 ? grad_feats + (size_t)r * C + c4 : partial + interp_backward_slot(first, r, j) * C + c4;
  *reinterpret_cast<float4*>(dst) = acc;
}

// rows of more than one chunk: their partial sums in chunk order
__global__ __launch_bounds__(256) void interp_backward_combine_kernel(const int* __restrict__ chunk_ofs, int n_in, int C,
                                                                      const float* __restrict__ partial,
                                                                      float* __restrict__ grad_feats) {
  const int tpc = C / 4, sh = __builtin_ctz(tpc);
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const int r = (int)(gid >> sh), c4 = (int)(gid & (tpc - 1)) * 4;
  if (r >= n_in) return;
  const int first = chunk_ofs[r], nch = chunk_ofs[r + 1] - first;
  if (nch == 1) return;
  const float* p = partial + interp_backward_slot(first, r, 0) * C + c4;
  float4 acc = *reinterpret_cast<const float4*>(p);
  for (int j = 1; j < nch; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(p + (size_t)j * C);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<float4*>(grad_feats + (size_t)r * C + c4) = acc;
}

size_t interp_backward_scan_bytes(int n) {
  size_t b = 0;
  int* p = nullptr;
  (void)rocprim::exclusive_scan(nullptr, b, p, p, 0, (size_t)n, rocprim::plus<int>(), (hipStream_t)0);
  return v3d::align_up(b, 256);
}

// workspace: [crow n*4][cw n*4][perm n*4][offsets (n_in+2)*4][nch (n_in+1)*4][chunk_ofs (n_in+1)*4][partial][scan temp][csr]
struct InterpBackwardLayout {
  size_t cw, perm, offsets, nch, chunk_ofs, partial, scan, scan_bytes, csr, csr_bytes, total;
  InterpBackwardLayout(int n_in, int C, long long n) {
    const size_t slots = v3d::align_up((size_t)n * 4, 256), rows = v3d::align_up(((size_t)n_in + 2) * 4, 256);
    cw = slots;
    perm = cw + slots;
    offsets = perm + slots;
    nch = offsets + rows;
    chunk_ofs = nch + rows;
    partial = chunk_ofs + rows;
    scan = partial + v3d::align_up((2 * (size_t)(n / kInterpBwdChunk) + 2) * C * 4, 256);
    scan_bytes = interp_backward_scan_bytes(n_in + 1);
    csr = scan + scan_bytes;
    csr_bytes = v3d_segment_csr_workspace_bytes((int)n);
    total = csr + csr_bytes;
  }
};

// What v3d_sparse_interp_f32 (`fn`) and its backward share: the checks of the level, the queries and the workspace of `need` bytes,
// then -- unless there is no query: nq = 0, nothing launched -- the corner table at the head of the workspace ([crow nq*8*4][cw
// nq*8*4], 256-byte aligned sections; row -1 = absent corner), launched inside the timed scope `scope`, which stays open as long
// as `ct.timed` lives.  `own_args` / `own_shape`: the caller's pointers are there / its leading dimensions fit.
struct CornerTable { long long nq; int* crow; float* cw; std::optional<v3d::TimedScope> timed; };
int interp_corner_table(const char* fn, const char* scope, bool own_args, bool own_shape, const void* table, int n_in, int C,
                        int tensor_stride, const float* pts, const int64_t* pts_batch, int n_pts, int n_hyp, const float* min_pts,
                        float res, void* workspace, size_t workspace_bytes, size_t need, hipStream_t s, CornerTable& ct) {
  V3D_REQUIRE(table && pts && pts_batch && min_pts && own_args, V3D_ERR_BAD_ARG, "%s: null argument", fn);
  V3D_REQUIRE(C % 4 == 0 && C >= 4 && C <= 1024 && 256 % (C / 4) == 0, V3D_ERR_UNSUPPORTED, "%s: C=%d unsupported", fn, C);
  V3D_REQUIRE(n_in > 0 && n_pts >= 0 && n_hyp > 0 && tensor_stride > 0 && res > 0.f && own_shape, V3D_ERR_BAD_SHAPE, "%s: bad shape", fn);
  const long long nq = ct.nq = (long long)n_pts * n_hyp;
  if (nq == 0) return V3D_OK;
  V3D_REQUIRE(nq * 8 < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: too many queries", fn);
  V3D_REQUIRE(workspace && workspace_bytes >= need, V3D_ERR_WORKSPACE_TOO_SMALL, "%s: workspace too small", fn);
  ct.crow = (int*)workspace;
  ct.cw = (float*)((char*)workspace + v3d::align_up((size_t)nq * 8 * 4, 256));
  const Level L = level_view(table, n_in, min_pts, res, tensor_stride);
  const long long* pb = (const long long*)pts_batch;
  ct.timed.emplace(scope, s);
  if (stride_is_pow2(tensor_stride))
    interp_corners_kernel<true><<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(L, pts, pb, n_hyp, (int)nq, ct.crow, ct.cw);
  else
    interp_corners_kernel<false><<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(L, pts, pb, n_hyp, (int)nq, ct.crow, ct.cw);
  return V3D_OK;
}

}  // namespace

int v3dinterp::launch_decoder_corners(const Level (&levels)[3], bool pow2, const float* pts, const int64_t* pts_batch, int n_pts,
                                      int n_hyp, void* out, hipStream_t s) {
  const int n_q = n_pts * n_hyp;
  const CornerParams cp{{levels[0], levels[1], levels[2]}, pts, (const long long*)pts_batch, n_hyp,
                        v3d::magic_u32((unsigned long long)n_q, (unsigned)n_hyp), n_q, reinterpret_cast<u32x2*>(out)};
  const long long n_thr = (long long)n_q * 8;
  v3d::TimedScope ts("decoder_corners", s);
  if (pow2) decoder_corner_kernel<true><<<(unsigned)((n_thr + 255) / 256), 256, 0, s>>>(cp);
  else decoder_corner_kernel<false><<<(unsigned)((n_thr + 255) / 256), 256, 0, s>>>(cp);
  V3D_CHECK_LAUNCH("decoder_corner_kernel");
  return V3D_OK;
}

#ifdef V3D_CORNER_STATS
extern "C" int v3d_debug_corner_stats(unsigned long long* out12, int reset) {
  if (hipMemcpyFromSymbol(out12, HIP_SYMBOL(g_corner_stats), sizeof(unsigned long long) * 12) != hipSuccess) return 1;
  if (reset) { unsigned long long z[12] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_corner_stats), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif

extern "C" size_t v3d_sparse_interp_workspace_bytes(int n_pts, int n_hyp) {
  return v3d::align_up((size_t)n_pts * n_hyp * 8 * 4, 256) * 2;
}

extern "C" int v3d_sparse_interp_f32(const void* table, int n_in, const float* feats, int C, int tensor_stride, const float* pts,
                                     const int64_t* pts_batch, int n_pts, int n_hyp, const float* min_pts, float res, float* out,
                                     int ld_out, int col0, void* workspace, size_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CornerTable ct;
  const int rc = interp_corner_table("v3d_sparse_interp_f32", "sparse_interp", feats && out, true, table, n_in, C, tensor_stride, pts,
                                     pts_batch, n_pts, n_hyp, min_pts, res, workspace, workspace_bytes,
                                     v3d_sparse_interp_workspace_bytes(n_pts, n_hyp), s, ct);
  if (rc != V3D_OK || ct.nq == 0) return rc;
  const long long threads = ct.nq * (C / 4);
  interp_gather_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(feats, C, ct.crow, ct.cw, (int)ct.nq, out, ld_out, col0);
  V3D_CHECK_LAUNCH("interp_gather_kernel");
  return V3D_OK;
}

extern "C" size_t v3d_sparse_interp_backward_workspace_bytes(int n_in, int C, int n_pts, int n_hyp) {
  const long long n = (long long)n_pts * n_hyp * 8;
  if (n_in <= 0 || C <= 0 || n <= 0 || n >= (1ll << 31)) return 256;
  return InterpBackwardLayout(n_in, C, n).total;
}

extern "C" int v3d_sparse_interp_backward_f32(const void* table, int n_in, int C, int tensor_stride, const float* pts,
                                              const int64_t* pts_batch, int n_pts, int n_hyp, const float* min_pts, float res,
                                              const float* grad_out, int ld_grad, int col0, float* grad_feats, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  const char* const fn = "v3d_sparse_interp_backward_f32";
  V3D_REQUIRE((reinterpret_cast<size_t>(grad_feats) & 15) == 0, V3D_ERR_BAD_ARG,
              "%s: grad_feats must be 16-byte aligned (its rows are stored as float4)", fn);
  hipStream_t s = (hipStream_t)stream;
  CornerTable ct;
  int rc = interp_corner_table(fn, "sparse_interp_backward_corners", grad_out && grad_feats,
                               col0 >= 0 && (long long)ld_grad >= (long long)col0 + C, table, n_in, C, tensor_stride, pts, pts_batch,
                               n_pts, n_hyp, min_pts, res, workspace, workspace_bytes,
                               v3d_sparse_interp_backward_workspace_bytes(n_in, C, n_pts, n_hyp), s, ct);
  if (rc != V3D_OK) return rc;
  const long long nq = ct.nq;
  if (nq == 0) {
    V3D_CHECK_HIP(hipMemsetAsync(grad_feats, 0, (size_t)n_in * C * sizeof(float), s));
    return V3D_OK;
  }
  const int n = (int)(nq * 8), tpc = C / 4;
  int* const crow = ct.crow;
  const float* const cw = ct.cw;
  interp_backward_segment_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(crow, n, n_in);
  ct.timed.reset();                      // "sparse_interp_backward_corners" ends here
  V3D_CHECK_LAUNCH("interp_backward_segment_kernel");
  const InterpBackwardLayout L(n_in, C, n);
  char* base = (char*)workspace;
  int *perm = (int*)(base + L.perm), *offsets = (int*)(base + L.offsets), *nch = (int*)(base + L.nch);
  int* chunk_ofs = (int*)(base + L.chunk_ofs);
  float* partial = (float*)(base + L.partial);
  rc = v3d_segment_csr(crow, n, n_in + 1, perm, offsets, base + L.csr, L.csr_bytes, s);
  if (rc != V3D_OK) return rc;
  v3d::TimedScope ts("sparse_interp_backward", s);
  interp_backward_count_kernel<<<(unsigned)(((long long)n_in + 256) / 256), 256, 0, s>>>(offsets, n_in, nch);
  size_t scan_bytes = L.scan_bytes;
  V3D_CHECK_HIP(rocprim::exclusive_scan(base + L.scan, scan_bytes, nch, chunk_ofs, 0, (size_t)n_in + 1, rocprim::plus<int>(), s));
  const long long max_chunks = (long long)(n / kInterpBwdChunk) + n_in;      // the static bound of chunk_ofs[n_in]
  const unsigned blocks = (unsigned)((max_chunks * tpc + 255) / 256);
  const bool vec = (reinterpret_cast<size_t>(grad_out) & 15) == 0 && ld_grad % 4 == 0 && col0 % 4 == 0;
  if (vec)
    interp_backward_chunk_kernel<true><<<blocks, 256, 0, s>>>(perm, offsets, chunk_ofs, n_in, C, cw, grad_out, ld_grad, col0,
                                                             grad_feats, partial);
  else
    interp_backward_chunk_kernel<false><<<blocks, 256, 0, s>>>(perm, offsets, chunk_ofs, n_in, C, cw, grad_out, ld_grad, col0,
                                                              grad_feats, partial);
  interp_backward_combine_kernel<<<(unsigned)(((long long)n_in * tpc + 255) / 256), 256, 0, s>>>(chunk_ofs, n_in, C, partial,
                                                                                                grad_feats);
  V3D_CHECK_LAUNCH("interp_backward_combine_kernel");
  return V3D_OK;
}
