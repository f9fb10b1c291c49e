// Training of row B4: what the backward of PointNet's per-voxel max pooling and of cat(x, pool[idx]) needs beside
// dense products.  Three streaming kernels in the launch shape of segment_max_kernel (segment.hip): LPS lanes x float4 per row,
// 256 / LPS rows per workgroup, whole rows gathered through the row list of v3d_segment_csr.  No LDS, no atomics, one fixed order
// of additions: two calls give the same bits.
#include "v3d_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The walk of segment_max_kernel with the winner's ROW beside the maximum.  The values go through the very max chains of that
// kernel (the same bits); a row takes a chain's slot when it beats the chain's maximum strictly, or when the slot is still free
// and the value is no NaN (so a NaN never wins and a segment of -inf rows still names one).  Rows ascend along a segment's list
// (the sort is stable), so "first on strict >" per chain and "the lower row on equal maxima" between the two chains is the lowest
// row among equal values.
__device__ __forceinline__ void take_winner(const f32x4& v, int row, const f32x4& m, i32x4& a) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (v[j] > m[j] || (a[j] < 0 && v[j] == v[j])) a[j] = row;
}

template <int LPS>
__global__ __launch_bounds__(256) void segment_max_arg_kernel(const float* __restrict__ src, int ld, const int* __restrict__ perm,
                                                              const int* __restrict__ offsets, int n_seg, int N,
                                                              float* __restrict__ out, int ld_out, int* __restrict__ arg,
                                                              int ld_arg) {
  const int seg = blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
  const int c = (threadIdx.x % LPS) * 4;
  if (seg >= n_seg || c >= N) return;
  const int r0 = offsets[seg], r1 = offsets[seg + 1];
  f32x4 m0 = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, m1 = m0;
  i32x4 a0 = {-1, -1, -1, -1}, a1 = a0;
  int r = r0;
  for (; r + 1 < r1; r += 2) {            // two independent row gathers in flight
    const int pa = perm[r], pb = perm[r + 1];
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)pa * ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + (size_t)pb * ld + c);
    take_winner(a, pa, m0, a0);
    take_winner(b, pb, m1, a1);
    m0 = __builtin_elementwise_max(m0, a);
    m1 = __builtin_elementwise_max(m1, b);
  }
  if (r < r1) {
    const int pa = perm[r];
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)pa * ld + c);
    take_winner(a, pa, m0, a0);
    m0 = __builtin_elementwise_max(m0, a);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (a1[j] >= 0 && (a0[j] < 0 || m1[j] > m0[j] || (m1[j] == m0[j] && a1[j] < a0[j]))) a0[j] = a1[j];
  *reinterpret_cast<f32x4*>(out + (size_t)seg * ld_out + c) = __builtin_elementwise_max(m0, m1);
  *reinterpret_cast<i32x4*>(arg + (size_t)seg * ld_arg + c) = a0;
}

// out[seg] = (the rows at the even positions of the list, added in list order to +0) + (the rows at its odd positions, likewise)
template <int LPS>
__global__ __launch_bounds__(256) void segment_sum_kernel(const float* __restrict__ src, int ld, const int* __restrict__ perm,
                                                          const int* __restrict__ offsets, int n_seg, int N,
                                                          float* __restrict__ out, int ld_out) {
  const int seg = blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
  const int c = (threadIdx.x % LPS) * 4;
  if (seg >= n_seg || c >= N) return;
  const int r0 = offsets[seg], r1 = offsets[seg + 1];
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  int r = r0;
  for (; r + 1 < r1; r += 2) {            // two independent row gathers in flight
    const f32x4 a = *reinterpret_cast<const f32x4*>(src + (size_t)perm[r] * ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(src + (size_t)perm[r + 1] * ld + c);
    s0 += a;
    s1 += b;
  }
  if (r < r1) s0 += *reinterpret_cast<const f32x4*>(src + (size_t)perm[r] * ld + c);
  *reinterpret_cast<f32x4*>(out + (size_t)seg * ld_out + c) = s0 + s1;
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
  const int row = blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
  const int c = (threadIdx.x % LPS) * 4;
  if (row >= p.n || c >= p.N) return;
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

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool row_shape_ok(int N, int ld) { return N > 0 && N % 4 == 0 && N <= 256 && ld % 4 == 0 && ld >= N; }

// the launch shape of segment_max_kernel: 32 lanes x float4 per row of up to 128 columns, 64 up to 256
#define V3D_ROW_LAUNCH(kernel32, kernel64, rows, ...)                                           \
  do {                                                                                          \
    if (N <= 128) kernel32<<<((rows) + 7) / 8, 256, 0, s>>>(__VA_ARGS__);                       \
    else kernel64<<<((rows) + 3) / 4, 256, 0, s>>>(__VA_ARGS__);                                \
  } while (0)

}  // namespace

extern "C" int v3d_segment_max_arg_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N,
                                       float* out, int ld_out, int32_t* arg, int ld_arg, void* stream) {
  V3D_REQUIRE(src && perm && offsets && out && arg, V3D_ERR_BAD_ARG, "v3d_segment_max_arg_f32: null argument");
  V3D_REQUIRE(aligned16(src) && aligned16(out) && aligned16(arg), V3D_ERR_BAD_ARG,
              "v3d_segment_max_arg_f32: src, out and arg must be 16-byte aligned");
  V3D_REQUIRE(n_seg > 0 && row_shape_ok(N, ld) && row_shape_ok(N, ld_out) && row_shape_ok(N, ld_arg), V3D_ERR_BAD_SHAPE,
              "v3d_segment_max_arg_f32: n_seg=%d N=%d ld=%d ld_out=%d ld_arg=%d (N a multiple of 4, <= 256)", n_seg, N, ld, ld_out,
              ld_arg);
  hipStream_t s = (hipStream_t)stream;
  v3d::TimedScope ts("segment_max_arg", s);
  V3D_ROW_LAUNCH(segment_max_arg_kernel<32>, segment_max_arg_kernel<64>, n_seg, src, ld, perm, offsets, n_seg, N, out, ld_out, arg,
                 ld_arg);
  V3D_CHECK_LAUNCH("segment_max_arg_kernel");
  return V3D_OK;
}

extern "C" int v3d_segment_sum_f32(const float* src, int ld, const int32_t* perm, const int32_t* offsets, int n_seg, int N,
                                   float* out, int ld_out, void* stream) {
  V3D_REQUIRE(src && perm && offsets && out, V3D_ERR_BAD_ARG, "v3d_segment_sum_f32: null argument");
  V3D_REQUIRE(aligned16(src) && aligned16(out), V3D_ERR_BAD_ARG, "v3d_segment_sum_f32: src and out must be 16-byte aligned");
  V3D_REQUIRE(n_seg > 0 && row_shape_ok(N, ld) && row_shape_ok(N, ld_out), V3D_ERR_BAD_SHAPE,
              "v3d_segment_sum_f32: n_seg=%d N=%d ld=%d ld_out=%d (N a multiple of 4, <= 256)", n_seg, N, ld, ld_out);
  hipStream_t s = (hipStream_t)stream;
  v3d::TimedScope ts("segment_sum", s);
  V3D_ROW_LAUNCH(segment_sum_kernel<32>, segment_sum_kernel<64>, n_seg, src, ld, perm, offsets, n_seg, N, out, ld_out);
  V3D_CHECK_LAUNCH("segment_sum_kernel");
  return V3D_OK;
}

extern "C" int v3d_pointnet_pool_backward_f32(const float* grad_lin, int ld_lin, const float* x, int ld_x, const int32_t* seg_id,
                                              const float* grad_pool, int ld_pool, const int32_t* arg, int ld_arg, int n, int N,
                                              float* grad_x, int ld_gx, void* stream) {
  V3D_REQUIRE(seg_id && grad_pool && arg && grad_x && (!grad_lin || x), V3D_ERR_BAD_ARG,
              "v3d_pointnet_pool_backward_f32: null argument (x may be null only with grad_lin)");
  V3D_REQUIRE(aligned16(grad_lin) && (!grad_lin || aligned16(x)) && aligned16(grad_pool) && aligned16(arg) && aligned16(grad_x),
              V3D_ERR_BAD_ARG, "v3d_pointnet_pool_backward_f32: the matrices must be 16-byte aligned");
  V3D_REQUIRE(n > 0 && row_shape_ok(N, ld_pool) && row_shape_ok(N, ld_arg) && row_shape_ok(N, ld_gx) &&
                  (!grad_lin || (row_shape_ok(N, ld_lin) && row_shape_ok(N, ld_x))),
              V3D_ERR_BAD_SHAPE, "v3d_pointnet_pool_backward_f32: n=%d N=%d ld_lin=%d ld_x=%d ld_pool=%d ld_arg=%d ld_gx=%d (N a "
              "multiple of 4, <= 256)", n, N, ld_lin, ld_x, ld_pool, ld_arg, ld_gx);
  hipStream_t s = (hipStream_t)stream;
  v3d::TimedScope ts("pointnet_pool_backward", s);
  const PoolBackwardArgs p = {grad_lin, ld_lin, grad_lin ? x : nullptr, ld_x, seg_id, grad_pool, ld_pool, arg, ld_arg, n, N, grad_x,
                              ld_gx};
  const auto k32 = grad_lin ? pointnet_pool_backward_kernel<32, 1> : pointnet_pool_backward_kernel<32, 0>;
  const auto k64 = grad_lin ? pointnet_pool_backward_kernel<64, 1> : pointnet_pool_backward_kernel<64, 0>;
  V3D_ROW_LAUNCH(k32, k64, n, p);
  V3D_CHECK_LAUNCH("pointnet_pool_backward_kernel");
  return V3D_OK;
}
