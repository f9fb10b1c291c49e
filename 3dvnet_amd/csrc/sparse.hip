// Hash-indexed sparse-tensor structure kernels replacing MinkowskiEngine's coordinate manager on the
// refinement path (semantics restated in SURVEY Appendix A):
//   * open-addressing hash table over packed (batch, x, y, z) coordinates,
//   * 27-offset neighbour ("kernel map") tables for stride-1 / stride-2 convs and stride-2 transposed
//     convs -- consumed as row maps by the gather-GEMM (gemm_gather.hip),
//   * sparse trilinear interpolation at arbitrary query points (MinkowskiInterpolation,
//     mv3d/subnetworks/refinement.py:26,39), written straight into the decoder's wide feature row.
#include "sparse_hash.h"

namespace {

using namespace v3dhash;

__global__ void hash_clear_kernel(HashEntry* entries, unsigned cap, int* status) {
  unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap) entries[i] = HashEntry{kEmpty, -1, 0};
  if (i == 0) *status = 0;
}

__global__ void hash_insert_kernel(HashTable t, const int* __restrict__ coords, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cb = coords[i * 4], cx = coords[i * 4 + 1], cy = coords[i * 4 + 2], cz = coords[i * 4 + 3];
  if (cb < 0 || cb > 65535 || min(cx, min(cy, cz)) < -kGuard || max(cx, max(cy, cz)) > kCoordMax) {
    atomicOr(t.status, 1);          // would alias another key: reported by v3d_hash_status, row left out
    return;
  }
  const unsigned long long key = pack_key(cb, cx, cy, cz);
  unsigned slot = hash_u64(key) & t.mask;
  for (unsigned probe = 0; probe <= t.mask; ++probe) {
    const unsigned long long prev = atomicCAS(&t.entries[slot].key, kEmpty, key);
    if (prev == kEmpty || prev == key) { t.entries[slot].val = i; return; }   // coordinates are unique rows
    slot = (slot + 1) & t.mask;
  }
}

// nbr[k][p] = row of (out_coords[p] + step * o_k) in the hashed map, o_k in {-1,0,1}^3 with
// k = (ox+1) + 3 (oy+1) + 9 (oz+1);  conv: step = +ts_in, transposed conv: step = -ts_out.
// One thread per (offset, output row): the 27 probes of a row were a loop in one thread -- 27 dependent probe chains in a row,
// 40-50 us per launch whatever the level's size (2.8 k rows took as long as 60 k).  blockIdx.y = offset k, so a wave's stores
// are 64 consecutive ints of column k.
__global__ void neighbors_kernel(HashTable t, const int* __restrict__ out_coords, int n_out, int step,
                                 int* __restrict__ nbr) {
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (i >= n_out) return;
  const int4 c = *reinterpret_cast<const int4*>(out_coords + (size_t)i * 4);      // (batch, x, y, z)
  const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;
  nbr[(size_t)k * n_out + i] = hash_find(t, pack_key(c.x, c.y + step * ox, c.z + step * oy, c.w + step * oz));
}

// Sparse trilinear interpolation in two kernels:
//  1. corners: one thread per (query, corner) -- the 8 hash probes of a query run in parallel lanes and
//     leave (row, weight) pairs in a small scratch table (row -1 = absent corner, weight unused);
//  2. gather:  C/4 threads per query, float4 channels each; the 8 feature-row loads are independent
//     (no probe in between), so they are all in flight together.
__global__ __launch_bounds__(256) void interp_corners_kernel(HashTable t, int ts, const float* __restrict__ pts,
                                                             const long long* __restrict__ pts_batch, int n_hyp,
                                                             const float* __restrict__ min_pts, float res,
                                                             int n_query, int* __restrict__ crow,
                                                             float* __restrict__ cw) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int q = gid >> 3, corner = gid & 7;
  if (q >= n_query) return;
  const int b = (int)pts_batch[q / n_hyp];
  // query coordinate in base-voxel units: ((p - min) / x.res) * x.stride   (refinement.py:34-35)
  float w = 1.f;
  float cc[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float qc = ((pts[(size_t)q * 3 + d] - min_pts[b * 3 + d]) / res) * (float)ts;
    const float c = floorf(qc / (float)ts) * (float)ts + (((corner >> d) & 1) ? ts : 0);
    w *= 1.f - fabsf(qc - c) / ts;
    cc[d] = c;
  }
  int row = -1;
  // coordinates far outside the packed range cannot be present
  if (cc[0] >= -kGuard && cc[1] >= -kGuard && cc[2] >= -kGuard && cc[0] <= 60000.f && cc[1] <= 60000.f && cc[2] <= 60000.f)
    row = hash_find(t, pack_key(b, (int)cc[0], (int)cc[1], (int)cc[2]));
  crow[gid] = row;
  cw[gid] = w;
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

}  // namespace

extern "C" size_t v3d_hash_bytes(int n) { return (size_t)table_capacity(n) * sizeof(HashEntry) + 16; }

extern "C" int v3d_hash_status(const void* table, int n, void* stream) {
  V3D_REQUIRE(table && n > 0, V3D_ERR_BAD_ARG, "v3d_hash_status: bad argument");
  HashTable t = table_view(const_cast<void*>(table), n);
  int st = 0;
  V3D_CHECK_HIP(hipMemcpyAsync(&st, t.status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  V3D_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  V3D_REQUIRE(st == 0, V3D_ERR_BAD_SHAPE,
              "v3d_hash_build: a coordinate is outside the packed-key range (batch 0..65535, x/y/z %d..%d)", -kGuard,
              kCoordMax);
  return V3D_OK;
}

extern "C" int v3d_hash_build(const int32_t* coords, int n, void* table, size_t table_bytes, void* stream) {
  V3D_REQUIRE(coords && table, V3D_ERR_BAD_ARG, "v3d_hash_build: null argument");
  V3D_REQUIRE(n > 0, V3D_ERR_BAD_SHAPE, "v3d_hash_build: empty coordinate map");
  V3D_REQUIRE(table_bytes >= v3d_hash_bytes(n), V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_hash_build: table buffer too small");
  hipStream_t s = (hipStream_t)stream;
  HashTable t = table_view(table, n);
  v3d::TimedScope ts("hash_build", s);
  hash_clear_kernel<<<(t.mask + 256) / 256, 256, 0, s>>>(t.entries, t.mask + 1, t.status);
  hash_insert_kernel<<<(n + 255) / 256, 256, 0, s>>>(t, coords, n);
  V3D_CHECK_LAUNCH("hash_insert_kernel");
  return V3D_OK;
}

extern "C" int v3d_sparse_neighbors(const void* table, int n_in, const int32_t* out_coords, int n_out,
                                    int step, int32_t* nbr, void* stream) {
  V3D_REQUIRE(table && out_coords && nbr, V3D_ERR_BAD_ARG, "v3d_sparse_neighbors: null argument");
  V3D_REQUIRE(n_in > 0 && n_out > 0 && step != 0, V3D_ERR_BAD_SHAPE, "v3d_sparse_neighbors: bad shape");
  V3D_REQUIRE((reinterpret_cast<size_t>(out_coords) & 15) == 0, V3D_ERR_BAD_ARG,
              "v3d_sparse_neighbors: out_coords must be 16-byte aligned (the kernel loads a coordinate row as one int4)");
  hipStream_t s = (hipStream_t)stream;
  HashTable t = table_view(const_cast<void*>(table), n_in);
  v3d::TimedScope ts("sparse_neighbors", s);
  neighbors_kernel<<<dim3((n_out + 255) / 256, 27), 256, 0, s>>>(t, out_coords, n_out, step, nbr);
  V3D_CHECK_LAUNCH("neighbors_kernel");
  return V3D_OK;
}

extern "C" size_t v3d_sparse_interp_workspace_bytes(int n_pts, int n_hyp) {
  return v3d::align_up((size_t)n_pts * n_hyp * 8 * 4, 256) * 2;
}

extern "C" int v3d_sparse_interp_f32(const void* table, int n_in, const float* feats, int C,
                                     int tensor_stride, const float* pts, const int64_t* pts_batch,
                                     int n_pts, int n_hyp, const float* min_pts, float res, float* out,
                                     int ld_out, int col0, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  V3D_REQUIRE(table && feats && pts && pts_batch && min_pts && out, V3D_ERR_BAD_ARG,
              "v3d_sparse_interp_f32: null argument");
  V3D_REQUIRE(C % 4 == 0 && C >= 4 && C <= 1024 && 256 % (C / 4) == 0, V3D_ERR_UNSUPPORTED,
              "v3d_sparse_interp_f32: C=%d unsupported", C);
  V3D_REQUIRE(n_in > 0 && n_pts >= 0 && n_hyp > 0 && tensor_stride > 0 && res > 0.f, V3D_ERR_BAD_SHAPE,
              "v3d_sparse_interp_f32: bad shape");
  const long long nq = (long long)n_pts * n_hyp;
  if (nq == 0) return V3D_OK;
  hipStream_t s = (hipStream_t)stream;
  HashTable t = table_view(const_cast<void*>(table), n_in);
  V3D_REQUIRE(workspace && workspace_bytes >= v3d_sparse_interp_workspace_bytes(n_pts, n_hyp),
              V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_sparse_interp_f32: workspace too small");
  V3D_REQUIRE(nq * 8 < (1ll << 31), V3D_ERR_BAD_SHAPE, "v3d_sparse_interp_f32: too many queries");
  int* crow = (int*)workspace;
  float* cw = (float*)((char*)workspace + v3d::align_up((size_t)nq * 8 * 4, 256));
  const long long threads = nq * (C / 4);
  v3d::TimedScope ts("sparse_interp", s);
  interp_corners_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(
      t, tensor_stride, pts, (const long long*)pts_batch, n_hyp, min_pts, res, (int)nq, crow, cw);
  interp_gather_kernel<<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(feats, C, crow, cw, (int)nq, out, ld_out, col0);
  V3D_CHECK_LAUNCH("interp_gather_kernel");
  return V3D_OK;
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
#include <rocprim/rocprim.hpp>      // after v3d_common.h (<cstring>: rocprim's texture iterator calls the host memset)

namespace {

using namespace v3dhash;

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

}  // namespace

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
  V3D_REQUIRE(table && pts && pts_batch && min_pts && grad_out && grad_feats, V3D_ERR_BAD_ARG, "%s: null argument", fn);
  V3D_REQUIRE((reinterpret_cast<size_t>(grad_feats) & 15) == 0, V3D_ERR_BAD_ARG,
              "%s: grad_feats must be 16-byte aligned (its rows are stored as float4)", fn);
  V3D_REQUIRE(C % 4 == 0 && C >= 4 && C <= 1024 && 256 % (C / 4) == 0, V3D_ERR_UNSUPPORTED, "%s: C=%d unsupported", fn, C);
  V3D_REQUIRE(n_in > 0 && n_pts >= 0 && n_hyp > 0 && tensor_stride > 0 && res > 0.f && col0 >= 0 &&
                  (long long)ld_grad >= (long long)col0 + C,
              V3D_ERR_BAD_SHAPE, "%s: bad shape", fn);
  hipStream_t s = (hipStream_t)stream;
  const long long nq = (long long)n_pts * n_hyp;
  if (nq == 0) {
    V3D_CHECK_HIP(hipMemsetAsync(grad_feats, 0, (size_t)n_in * C * sizeof(float), s));
    return V3D_OK;
  }
  V3D_REQUIRE(nq * 8 < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: too many queries", fn);
  V3D_REQUIRE(workspace && workspace_bytes >= v3d_sparse_interp_backward_workspace_bytes(n_in, C, n_pts, n_hyp),
              V3D_ERR_WORKSPACE_TOO_SMALL, "%s: workspace too small", fn);
  const int n = (int)(nq * 8), tpc = C / 4;
  const InterpBackwardLayout L(n_in, C, n);
  char* base = (char*)workspace;
  int* crow = (int*)base;
  float* cw = (float*)(base + L.cw);
  int *perm = (int*)(base + L.perm), *offsets = (int*)(base + L.offsets), *nch = (int*)(base + L.nch);
  int* chunk_ofs = (int*)(base + L.chunk_ofs);
  float* partial = (float*)(base + L.partial);
  HashTable t = table_view(const_cast<void*>(table), n_in);
  {
    v3d::TimedScope ts("sparse_interp_backward_corners", s);
    interp_corners_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(t, tensor_stride, pts, (const long long*)pts_batch, n_hyp,
                                                                      min_pts, res, (int)nq, crow, cw);
    interp_backward_segment_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256, 0, s>>>(crow, n, n_in);
    V3D_CHECK_LAUNCH("interp_backward_segment_kernel");
  }
  const int rc = v3d_segment_csr(crow, n, n_in + 1, perm, offsets, base + L.csr, L.csr_bytes, s);
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
