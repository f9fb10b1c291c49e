// Backward of the fused plane-sweep warp + variance (rows A1-A4; psv_variance.hip is the map of the forward) with respect to the features
// (v3d_psv_variance_backward_f32, include/v3d.h).  Reference semantics: the autograd of mvsnet.py:209-216.
//
// The kernel is variance_backward.h's walk over the depth planes of the sweep: one single-wave workgroup per (reference view,
// 64 / C plane-grid pixels, segment of kBDS planes).  Cameras and plane depths are data; the plane depth is the forward's
// psv_plane_depth, the upstream gradient lies as the forward writes the variance, [n_ref, C, D, h, w].
#include "variance_backward.h"

namespace {

constexpr int kBDS = 16;      // depth planes a wave walks (one depth segment)

struct PsvBwdParams : v3d::VarianceBwdParams {      // n_samples = D, gvar [n_ref, C, D, h, w]
  double z_start, z_step, z_end;
  __device__ __forceinline__ float sample_depth(int, int, int d, bool) const {
    return v3d::psv_plane_depth(d, n_samples, z_start, z_step, z_end);
  }
  template <int C>
  __device__ __forceinline__ size_t gvar_index(int r, int pixel, int d, int c) const {
    return (((size_t)r * C + c) * n_samples + d) * (h * w) + pixel;
  }
};

template <int C>
__global__ __launch_bounds__(64) void psv_variance_backward_kernel(PsvBwdParams p) {
  v3d::variance_backward_walk<C, kBDS>(p);
}

}  // namespace

extern "C" int v3d_psv_variance_backward_f32(const float* feat_cl, const float* K, const float* R, const float* t,
                                             const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                             int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                             double depth_start, double depth_interval, int D, int h, int w,
                                             const float* grad_var, float* grad_feat_cl, void* stream) {
  const char* const fn = "v3d_psv_variance_backward_f32";
  V3D_REQUIRE(feat_cl && K && R && t && ref_img && edge_ofs && edge_src && grad_var && grad_feat_cl, V3D_ERR_BAD_ARG,
              "%s: null pointer argument", fn);
  if (const int rc = v3d::variance_backward_limits(fn, n_img, n_ref, n_edges, C, Hf, Wf, H, W, h, w, D > 0)) return rc;
  hipStream_t s = (hipStream_t)stream;
  V3D_CHECK_HIP(v3d::variance_backward_zero_fill(grad_feat_cl, n_img, Hf, Wf, C, s));

  PsvBwdParams p;
  p.feat = feat_cl; p.K = K; p.R = R; p.t = t;
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src; p.gvar = grad_var; p.gfeat = grad_feat_cl;
  const long long blocks = v3d::variance_backward_geometry(p, n_ref, C, Hf, Wf, H, W, h, w, D, kBDS);
  const double depth_end = depth_start + (double)(D - 1) * depth_interval;
  p.z_start = depth_start;
  p.z_step = D > 1 ? (depth_end - depth_start) / (double)(D - 1) : 0.0;
  p.z_end = depth_end;
  V3D_REQUIRE(blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: grid too large", fn);
  {
    v3d::TimedScope ts("psv_variance_backward", s);
    if (C == 32) psv_variance_backward_kernel<32><<<(unsigned)blocks, 64, 0, s>>>(p);
    else psv_variance_backward_kernel<16><<<(unsigned)blocks, 64, 0, s>>>(p);
  }
  V3D_CHECK_LAUNCH("psv_variance_backward_kernel");
  return V3D_OK;
}
