// Plane-sweep warp + variance: what runs in front of the warp kernels (psv_variance.hip is the map of the family) -- the
// channel-last copies of the feature maps, the per-image camera blocks -- and the diagnostic twin of the kernels' projection.
#include "psv_kernels.h"

namespace v3d {
namespace {

constexpr int kPix = 64;     // pixels / bordered cells per workgroup of the transposes

// [n_img, C, HW] -> [n_img, HW, C]
template <int C>
__global__ __launch_bounds__(256) void transpose_channel_last_kernel(const float* __restrict__ in, float* __restrict__ out, int HW) {
  __shared__ float tile[C][kPix + 1];
  const int img = blockIdx.y;
  const int p0 = blockIdx.x * kPix;
  const float* src = in + (size_t)img * C * HW;
  float* dst = out + (size_t)img * HW * C;
  for (int i = threadIdx.x; i < C * kPix; i += 256) {
    int c = i / kPix, p = i % kPix;
    tile[c][p] = (p0 + p < HW) ? src[(size_t)c * HW + p0 + p] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * kPix; i += 256) {
    int p = i / C, c = i % C;
    if (p0 + p < HW) dst[(size_t)(p0 + p) * C + c] = tile[c][p];
  }
}

// [n_img, C, Hf, Wf] -> [n_img, Hf + 2, Wf + 2, C] with a border of zero cells (+ a tail of zero cells behind the last image).
// grid_sample's padding_mode='zeros' then needs no per-tap validity test in the warp kernels: a tap outside the image reads
// a zero cell, and a sample further out is clamped onto the border, where both of its in-range taps are zero cells and the
// other two carry weight 0 (make_taps).  One workgroup = 64 consecutive cells of one padded image.
template <int C>
__global__ __launch_bounds__(256) void transpose_bordered_kernel(const float* __restrict__ in, float* __restrict__ out, int Hf,
                                                                  int Wf, int n_img) {
  __shared__ float tile[C][kPix + 1];
  const int img = blockIdx.y;
  const int Wp = Wf + 2, HW = Hf * Wf, n_cell = (Hf + 2) * Wp;
  const int q0 = blockIdx.x * kPix;                      // 64 consecutive cells of the padded image (row-major)
  const float* src = in + (size_t)img * C * HW;
  float* dst = out + (size_t)img * n_cell * C;
  for (int i = threadIdx.x; i < C * kPix; i += 256) {
    const int c = i / kPix, q = q0 + i % kPix;
    const int yb = q / Wp, xb = q - yb * Wp;
    const bool inside = q < n_cell && yb >= 1 && yb <= Hf && xb >= 1 && xb <= Wf;
    tile[c][i % kPix] = inside ? src[(size_t)c * HW + (yb - 1) * Wf + xb - 1] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < C * kPix; i += 256) {
    const int px = i / C, c = i % C;
    if (q0 + px < n_cell) dst[(size_t)(q0 + px) * C + c] = tile[c][px];
  }
  // A sample clamped onto the lower border reads its weight-0 taps one padded row further down: the next image's top border,
  // or, behind the last image, this tail of zero cells.  Weight 0 times recycled memory holding a NaN pattern would be NaN.
  // The window kernel copies whole 8-cell runs of up to one row below a footprint: the tail is two bordered rows + 16 cells.
  if (img == n_img - 1 && blockIdx.x == 0) {
    float* tail = out + (size_t)n_img * n_cell * C;
    for (int i = threadIdx.x; i < kTailCells(Wf) * C; i += 256) tail[i] = 0.f;
  }
}

// Per-image camera blocks (psv_common.h, cam_block: K^-1, R, t, P = K [R|t]), one thread per image
__global__ void cam_setup_kernel(const float* __restrict__ K, const float* __restrict__ R,
                                 const float* __restrict__ t, float* __restrict__ camp, int n_img) {
  const int img = blockIdx.x * blockDim.x + threadIdx.x;
  if (img >= n_img) return;
  cam_block(K + img * 9, R + img * 9, t + img * 3, camp + img * kCamStride);
}

// Diagnostic twin of the warp kernels' projection (v3d_psv_sample_positions_f32): one thread per (edge, plane, pixel)
// runs the SAME device functions (v3d::world_point / v3d::sample_position) and stores the un-normalised sample position,
// so a test can compare the coordinates the kernels use with the reference's, bit for bit.
__global__ __launch_bounds__(256) void psv_positions_kernel(PsvParams p, float* __restrict__ pos, float* __restrict__ world) {
  const int P = p.h * p.w;
  const long long n_vox = (long long)p.D * P;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (i >= n_vox) return;
  const int d = (int)(i / P), gp = (int)(i % P), gy = gp / p.w, gx = gp % p.w;
  const float xf = psv_grid_coord(gx, p.w, p.W, p.x_step), yf = psv_grid_coord(gy, p.h, p.H, p.y_step);
  const float z = psv_plane_depth(d, p.D, p.z_start, p.z_step, p.z_end);
  float X, Y, Z;
  world_point(p.camp + p.ref_img[r] * kCamStride, xf, yf, z, X, Y, Z);
  if (world) {
    world[((size_t)r * 3 + 0) * n_vox + i] = X;
    world[((size_t)r * 3 + 1) * n_vox + i] = Y;
    world[((size_t)r * 3 + 2) * n_vox + i] = Z;
  }
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  const float rWm1 = (float)(1.0 / (double)(p.W - 1)), rHm1 = (float)(1.0 / (double)(p.H - 1));
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);
  for (int e = p.edge_ofs[r]; e < p.edge_ofs[r + 1]; ++e) {
    float ix, iy;
    sample_position(p.camp + p.edge_src[e] * kCamStride + 24, X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
    pos[((size_t)e * n_vox + i) * 2] = ix;
    pos[((size_t)e * n_vox + i) * 2 + 1] = iy;
  }
}

}  // namespace

// shared with backproject.hip
int transpose_channel_last(const float* feat, float* featT, int n_img, int C, int HW, hipStream_t s) {
  dim3 tg((HW + kPix - 1) / kPix, n_img);
  TimedScope ts("transpose_channel_last", s);
  if (C == 32) transpose_channel_last_kernel<32><<<tg, 256, 0, s>>>(feat, featT, HW);
  else if (C == 16) transpose_channel_last_kernel<16><<<tg, 256, 0, s>>>(feat, featT, HW);
  else return -1;
  return 0;
}

int launch_psv_prepare(const float* feat, const float* K, const float* R, const float* t, int n_img, int C, int Hf, int Wf,
                       float* featT, float* camp, hipStream_t s) {
  {
    TimedScope ts("transpose_channel_last", s);
    const dim3 tg(((Hf + 2) * (Wf + 2) + kPix - 1) / kPix, n_img);
    if (C == 32) transpose_bordered_kernel<32><<<tg, 256, 0, s>>>(feat, featT, Hf, Wf, n_img);
    else transpose_bordered_kernel<16><<<tg, 256, 0, s>>>(feat, featT, Hf, Wf, n_img);
  }
  V3D_CHECK_LAUNCH("transpose_bordered_kernel");
  cam_setup_kernel<<<(n_img + 63) / 64, 64, 0, s>>>(K, R, t, camp, n_img);
  V3D_CHECK_LAUNCH("cam_setup_kernel");
  return V3D_OK;
}

}  // namespace v3d

extern "C" int v3d_psv_sample_positions_f32(const float* K, const float* R, const float* t, const int32_t* ref_img,
                                            const int32_t* edge_ofs, const int32_t* edge_src, int n_img, int n_ref,
                                            int n_edges, int Hf, int Wf, int H, int W, double depth_start,
                                            double depth_interval, int D, int h, int w, float* pos, float* world,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  using v3d::kCamStride;
  V3D_REQUIRE(K && R && t && ref_img && edge_ofs && edge_src && pos && workspace, V3D_ERR_BAD_ARG,
              "v3d_psv_sample_positions_f32: null pointer argument");
  V3D_REQUIRE(n_img > 0 && n_ref > 0 && n_edges >= 0 && Hf > 0 && Wf > 0 && H > 1 && W > 1 && D > 0 && h > 0 && w > 0,
              V3D_ERR_BAD_SHAPE, "v3d_psv_sample_positions_f32: bad shape");
  V3D_REQUIRE(workspace_bytes >= (size_t)n_img * kCamStride * sizeof(float), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_psv_sample_positions_f32: workspace too small (n_img * 36 floats)");
  hipStream_t s = (hipStream_t)stream;
  float* camp = (float*)workspace;
  v3d::cam_setup_kernel<<<(n_img + 63) / 64, 64, 0, s>>>(K, R, t, camp, n_img);
  v3d::PsvParams p;
  memset(&p, 0, sizeof(p));
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src; p.camp = camp;
  p.n_img = n_img; p.n_ref = n_ref; p.Hf = Hf; p.Wf = Wf;
  v3d::psv_fill_grid(p, H, W, depth_start, depth_interval, D, h, w);
  const long long n_vox = (long long)D * h * w;
  v3d::psv_positions_kernel<<<dim3((unsigned)((n_vox + 255) / 256), n_ref), 256, 0, s>>>(p, pos, world);
  V3D_CHECK_LAUNCH("psv_positions_kernel");
  return V3D_OK;
}
