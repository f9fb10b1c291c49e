// Row B4's pooling (scenemodeling.py:129-141: scatter(x, idx, reduce='max') over the points of a voxel) without atomics, and what its
// training needs beside dense products: the winner rows, the per-voxel sums and the single-winner scatter.
// The gather-GEMM's fused scatter-max issues one atomic per (point, channel): 25.7 M of them per PointNet layer at cfg3, 0.43 of
// the layer's 0.53 ms, and twice that when the points of a voxel sit in consecutive rows (same address from neighbouring
// lanes).  Instead the points are grouped by voxel ONCE per forward (stable radix sort of (voxel id, row) -> row list + offsets,
// `v3d_segment_csr`), every layer stores its [M, N] output (it does anyway: the next layer reads it) and the row kernels below
// stream it: LPS lanes x float4 per row, 256 / LPS rows per workgroup, whole 512-byte rows gathered through the row list.  No LDS,
// no contention, one fixed order of operations: two calls give the same bits, and max, which is order independent, gives the
// atomic version's.  The lane mapping, the walk over a row list, the shape rule and the launch rule stand here once.
#include "v3d_common.h"      // <cstring> before rocprim: its texture iterator calls the host memset

#include <rocprim/rocprim.hpp>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void iota_kernel(unsigned* v, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = (unsigned)i;
}

// offsets[s] = first position of a key >= s in the sorted key list (binary search, one thread per segment; empty segments get
// an empty range); offsets[n_seg] = n
__global__ __launch_bounds__(256) void segment_offsets_kernel(const unsigned* __restrict__ sorted, int n, int n_seg,
                                                              int* __restrict__ offsets) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s > n_seg) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] < (unsigned)s) lo = mid + 1; else hi = mid;
  }
  offsets[s] = lo;
}

// this lane's row and the first of its four columns -> false: nothing to do
template <int LPS>
__device__ __forceinline__ bool row_lane(int rows, int N, int& row, int& c) {
  row = blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
  c = (threadIdx.x % LPS) * 4;
  return row < rows && c < N;
}

// A chain is what a lane carries along a row list: note(v, row) sees a gathered float4 before fold(v) takes it in.
struct MaxChain {
  f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  __device__ void note(const f32x4&, int) {}
  __device__ void fold(const f32x4& v) { m = __builtin_elementwise_max(m, v); }
  __device__ void merge(const MaxChain& o) { fold(o.m); }
};
struct SumChain {                                       // added in list order to +0
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  __device__ void note(const f32x4&, int) {}
  __device__ void fold(const f32x4& v) { s += v; }
  __device__ void merge(const SumChain& o) { fold(o.s); }
};
// MaxChain (so: its bits) with the winner's ROW beside each maximum.  A row takes a slot when it beats the slot's maximum strictly,
// or when the slot is still free and the value is no NaN (a NaN never wins; a segment of -inf rows still names one).  Rows ascend
// along a list (the sort is stable), so "first on strict >" per chain and "the lower row on equal maxima" between two chains is the
// lowest row among equal values.
struct MaxArgChain : MaxChain {
  i32x4 a = {-1, -1, -1, -1};
  __device__ void note(const f32x4& v, int row) {
    for (int j = 0; j < 4; ++j)
      if (v[j] > m[j] || (a[j] < 0 && v[j] == v[j])) a[j] = row;
  }
  __device__ void merge(const MaxArgChain& o) {
    for (int j = 0; j < 4; ++j)
      if (o.a[j] >= 0 && (a[j] < 0 || o.m[j] > m[j] || (o.m[j] == m[j] && o.a[j] < a[j]))) a[j] = o.a[j];
    fold(o.m);
  }
};

// This lane's segment and columns (false: none) and, in c0, columns c .. c + 3 of the segment's rows perm[offsets[seg] ..
// offsets[seg + 1]): c0 takes the even positions of the list and a second chain the odd ones, both gathers of a pair in flight and
// both noted before either is folded; an odd tail goes to c0, which last merges the second chain.
template <int LPS, class Chain>
__device__ __forceinline__ bool segment_walk(const float* src, int ld, const int* perm, const int* offsets, int n_seg, int N, int& seg,
                                             int& c, Chain& c0) {
  if (!row_lane<LPS>(n_seg, N, seg, c)) return false;
  const int r1 = offsets[seg + 1];
  Chain c1;
  int r = offsets[seg];
  for (; r + 1 < r1; r += 2) {
    const int pa = perm[r], pb = perm[r + 1];
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)pa * ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + (size_t)pb * ld + c);
    c0.note(a, pa);
    c1.note(b, pb);
    c0.fold(a);
    c1.fold(b);
  }
  if (r < r1) {
    const int pa = perm[r];
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)pa * ld + c);
    c0.note(a, pa);
    c0.fold(a);
  }
  c0.merge(c1);
  return true;
}

template <int LPS>
__global__ __launch_bounds__(256) void segment_max_kernel(const float* __restrict__ src, int ld, const int* __restrict__ perm,
                                                          const int* __restrict__ offsets, int n_seg, int N,
                                                          float* __restrict__ out, int ld_out) {
  int seg, c;
  MaxChain w;
  if (!segment_walk<LPS>(src, ld, perm, offsets, n_seg, N, seg, c, w)) return;
  *reinterpret_cast<f32x4*>(out + (size_t)seg * ld_out + c) = w.m;
}

template <int LPS>
__global__ __launch_bounds__(256) void segment_max_arg_kernel(const float* __restrict__ src, int ld, const int* __restrict__ perm,
                                                              const int* __restrict__ offsets, int n_seg, int N,
                                                              float* __restrict__ out, int ld_out, int* __restrict__ arg,
                                                              int ld_arg) {
  int seg, c;
  MaxArgChain w;
  if (!segment_walk<LPS>(src, ld, perm, offsets, n_seg, N, seg, c, w)) return;
  *reinterpret_cast<f32x4*>(out + (size_t)seg * ld_out + c) = w.m;
  *reinterpret_cast<i32x4*>(arg + (size_t)seg * ld_arg + c) = w.a;
}

// out[seg] = (the rows at the even positions of the list, added in list order to +0) + (the rows at its odd positions, likewise)
template <int LPS>
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ src, int ld, const int* __restrict__ perm,
                                                          const int* __restrict__ offsets, int n_seg, int N,
                                                          float* __restrict__ out, int ld_out) {
  int seg, c;
  SumChain w;
  if (!segment_walk<LPS>(src, ld, perm, offsets, n_seg, N, seg, c, w)) return;
  *reinterpret_cast<f32x4*>(out + (size_t)seg * ld_out + c) = w.s;
}

struct PoolBackwardArgs {
  const float* grad_lin; int ld_lin;
  const float* x; int ld_x;
  const int* seg_id;
  const float* grad_pool; int ld_pool;
  const int* arg; int ld_arg;
  int n, N;
  float* grad_x; int ld_gx;
};

// grad_x[r] = [x[r] > 0] grad_lin[r] + [arg[seg_id[r]] == r] grad_pool[seg_id[r]], every element written once; DIRECT = 0: the
// second term alone (the last pooling, whose x feeds only the pool)
template <int LPS, int DIRECT>
__global__ __launch_bounds__(256) void pointnet_pool_backward_kernel(const PoolBackwardArgs p) {
  int row, c;
  if (!row_lane<LPS>(p.n, p.N, row, c)) return;
  const int seg = p.seg_id[row];
  const f32x4 gp = *reinterpret_cast<const f32x4*>(p.grad_pool + (size_t)seg * p.ld_pool + c);
  const i32x4 a = *reinterpret_cast<const i32x4*>(p.arg + (size_t)seg * p.ld_arg + c);
  f32x4 g;
#pragma unroll
  for (int j = 0; j < 4; ++j) g[j] = a[j] == row ? gp[j] : 0.f;
  if (DIRECT) {
    const f32x4 gl = *reinterpret_cast<const f32x4*>(p.grad_lin + (size_t)row * p.ld_lin + c);
    const f32x4 xv = *reinterpret_cast<const f32x4*>(p.x + (size_t)row * p.ld_x + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = (xv[j] > 0.f ? gl[j] : 0.f) + g[j];
  }
  *reinterpret_cast<f32x4*>(p.grad_x + (size_t)row * p.ld_gx + c) = g;
}

// what the float4 accesses need of every matrix: its base and its row stride(s), N a multiple of 4 up to 64 lanes x 4
template <class... P>
bool aligned16(const P*... p) { return ((((uintptr_t)p & 15) == 0) && ...); }
template <class... L>
bool row_shape_ok(int N, L... ld) { return N > 0 && N % 4 == 0 && N <= 256 && ((ld % 4 == 0 && ld >= N) && ...); }

// the launch and its check: 32 lanes per row of up to 128 columns (8 rows per workgroup), 64 lanes up to 256 (4 rows per workgroup)
template <class K32, class K64, class... Args>
int launch_rows(const char* name, K32 kernel32, K64 kernel64, int rows, int N, void* stream, Args... args) {
  if (N <= 128) kernel32<<<(rows + 7) / 8, 256, 0, (hipStream_t)stream>>>(args...);
  else kernel64<<<(rows + 3) / 4, 256, 0, (hipStream_t)stream>>>(args...);
  V3D_CHECK_LAUNCH(name);
  return V3D_OK;
}

size_t sort_pairs_temp_bytes(int n) {
  size_t b = 0;
  unsigned* k = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, b, k, k, k, k, (size_t)n, 0, 32, (hipStream_t)0);
  return v3d::align_up(b, 256);
}

}  // namespace

// workspace: [sorted keys n*4][iota n*4][rocprim temp]
extern "C" size_t v3d_segment_csr_workspace_bytes(int n) {
  if (n <= 0) return 256;
  return 2 * v3d::align_up((size_t)n * 4, 256) + sort_pairs_temp_bytes(n);
}

extern "C" int v3d_segment_csr(const int32_t* seg_id, int n, int n_seg, int32_t* perm, int32_t* offsets, void* workspace,
                               size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(seg_id && perm && offsets && workspace, V3D_ERR_BAD_ARG, "v3d_segment_csr: null argument");
  V3D_REQUIRE(n > 0 && n_seg > 0, V3D_ERR_BAD_SHAPE, "v3d_segment_csr: n=%d n_seg=%d", n, n_seg);
  V3D_REQUIRE(workspace_bytes >= v3d_segment_csr_workspace_bytes(n), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_segment_csr: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  unsigned* sorted = (unsigned*)base;
  unsigned* iota = (unsigned*)(base + v3d::align_up((size_t)n * 4, 256));
  void* temp = base + 2 * v3d::align_up((size_t)n * 4, 256);
  size_t tb = sort_pairs_temp_bytes(n);
  v3d::TimedScope ts("segment_csr", s);
  iota_kernel<<<(n + 255) / 256, 256, 0, s>>>(iota, n);
  // ids are < n_seg: only the bits that can be set take part in the (stable) sort
  int bits = 1;
  while (bits < 32 && (1ll << bits) < (long long)n_seg) ++bits;
  V3D_CHECK_HIP(rocprim::radix_sort_pairs(temp, tb, (const unsigned*)seg_id, sorted, (const unsigned*)iota, (unsigned*)perm,
                                          (size_t)n, 0, bits, s));
  segment_offsets_kernel<<<(n_seg + 1 + 255) / 256, 256, 0, s>>>(sorted, n, n_seg, offsets);
  V3D_CHECK_LAUNCH("segment_offsets_kernel");
  return V3D_OK;
}

// (before v3d_segment_max_f32: instantiated in this order the compiler gives segment_max_arg_kernel 365 instructions, else 380)
extern "C" int v3d_segment_max_arg_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N,
                                       float* out, int ld_out, int32_t* arg, int ld_arg, void* stream) {
  V3D_REQUIRE(src && perm && offsets && out && arg, V3D_ERR_BAD_ARG, "v3d_segment_max_arg_f32: null argument");
  V3D_REQUIRE(aligned16(src, out, arg), V3D_ERR_BAD_ARG, "v3d_segment_max_arg_f32: src, out and arg must be 16-byte aligned");
  V3D_REQUIRE(n_seg > 0 && row_shape_ok(N, ld, ld_out, ld_arg), V3D_ERR_BAD_SHAPE,
              "v3d_segment_max_arg_f32: n_seg=%d N=%d ld=%d ld_out=%d ld_arg=%d (N a multiple of 4, <= 256)", n_seg, N, ld, ld_out,
              ld_arg);
  v3d::TimedScope ts("segment_max_arg", (hipStream_t)stream);
  return launch_rows("segment_max_arg_kernel", segment_max_arg_kernel<32>, segment_max_arg_kernel<64>, n_seg, N, stream, src, ld, perm,
                     offsets, n_seg, N, out, ld_out, arg, ld_arg);
}

extern "C" int v3d_segment_max_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N,
                                   float* out, int ld_out, void* stream) {
  V3D_REQUIRE(src && perm && offsets && out, V3D_ERR_BAD_ARG, "v3d_segment_max_f32: null argument");
  V3D_REQUIRE(aligned16(src, out), V3D_ERR_BAD_ARG, "v3d_segment_max_f32: src and out must be 16-byte aligned");
  V3D_REQUIRE(n_seg > 0 && row_shape_ok(N, ld, ld_out), V3D_ERR_BAD_SHAPE,
              "v3d_segment_max_f32: n_seg=%d N=%d ld=%d ld_out=%d (N a multiple of 4, <= 256)", n_seg, N, ld, ld_out);
  v3d::TimedScope ts("segment_max", (hipStream_t)stream);
  return launch_rows("segment_max_kernel", segment_max_kernel<32>, segment_max_kernel<64>, n_seg, N, stream, src, ld, perm, offsets,
                     n_seg, N, out, ld_out);
}

extern "C" int v3d_segment_sum_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N,
                                   float* out, int ld_out, void* stream) {
  V3D_REQUIRE(src && perm && offsets && out, V3D_ERR_BAD_ARG, "v3d_segment_sum_f32: null argument");
  V3D_REQUIRE(aligned16(src, out), V3D_ERR_BAD_ARG, "v3d_segment_sum_f32: src and out must be 16-byte aligned");
  V3D_REQUIRE(n_seg > 0 && row_shape_ok(N, ld, ld_out), V3D_ERR_BAD_SHAPE,
              "v3d_segment_sum_f32: n_seg=%d N=%d ld=%d ld_out=%d (N a multiple of 4, <= 256)", n_seg, N, ld, ld_out);
  v3d::TimedScope ts("segment_sum", (hipStream_t)stream);
  return launch_rows("segment_sum_kernel", segment_sum_kernel<32>, segment_sum_kernel<64>, n_seg, N, stream, src, ld, perm, offsets,
                     n_seg, N, out, ld_out);
}

extern "C" int v3d_pointnet_pool_backward_f32(const float* grad_lin, int ld_lin, const float* x, int ld_x, const int32_t* seg_id,
                                              const float* grad_pool, int ld_pool, const int32_t* arg, int ld_arg, int n, int N,
                                              float* grad_x, int ld_gx, void* stream) {
  V3D_REQUIRE(seg_id && grad_pool && arg && grad_x && (!grad_lin || x), V3D_ERR_BAD_ARG,
              "v3d_pointnet_pool_backward_f32: null argument (x may be null only with grad_lin)");
  V3D_REQUIRE(aligned16(grad_lin, grad_pool, arg, grad_x) && (!grad_lin || aligned16(x)), V3D_ERR_BAD_ARG,
              "v3d_pointnet_pool_backward_f32: the matrices must be 16-byte aligned");
  V3D_REQUIRE(n > 0 && row_shape_ok(N, ld_pool, ld_arg, ld_gx) && (!grad_lin || row_shape_ok(N, ld_lin, ld_x)), V3D_ERR_BAD_SHAPE,
              "v3d_pointnet_pool_backward_f32: n=%d N=%d ld_lin=%d ld_x=%d ld_pool=%d ld_arg=%d ld_gx=%d (N a multiple of 4, <= 256)",
              n, N, ld_lin, ld_x, ld_pool, ld_arg, ld_gx);
  v3d::TimedScope ts("pointnet_pool_backward", (hipStream_t)stream);
  const PoolBackwardArgs p = {grad_lin, ld_lin, grad_lin ? x : nullptr, ld_x, seg_id, grad_pool, ld_pool, arg, ld_arg, n, N, grad_x,
                              ld_gx};
  const char* name = "pointnet_pool_backward_kernel";
  if (grad_lin) return launch_rows(name, pointnet_pool_backward_kernel<32, 1>, pointnet_pool_backward_kernel<64, 1>, n, N, stream, p);
  return launch_rows(name, pointnet_pool_backward_kernel<32, 0>, pointnet_pool_backward_kernel<64, 0>, n, N, stream, p);
}
