// Backward of the back-projected variance (rows B1-B2 / C1; backproject.hip is the forward): v3d_backproject_variance_backward_f32,
// include/v3d.h.  Reference semantics: the autograd of mv3d/lightningmodel.py:132-174 (construct_feature_rich_pointcloud) and
// :187-235 (run_pointflow).  The reference builds the sampling grid under torch.no_grad() in both, so exactly two gradients exist:
//
//   var -> features (n_half >= 0).  Per reference view r with cnt edges, per pixel, hypothesis and channel:  x_e = bilinear sample
//     of source e (zeros padding), avg = sum_e x_e / cnt, var = sum_e x_e^2 / cnt - avg^2.  Given gV = dL/dvar:
//         g_e = gV * 2 * (x_e - avg) / cnt          dL/dfeat[src_e, tap, c] += w_tap * g_e   for the in-image taps.
//   pts -> depth (n_half == 0 only).  pts = R^T (K^-1 (p d) - t), p = (x, y, 1):  dL/dd = sum_j gP_j ray_j,  ray = R^T K^-1 p.
//
// The feature kernel is variance_backward.h's walk over the depth hypotheses of a pixel: single-wave workgroups, one per (reference
// view, 64 / C pixels, segment of S hypotheses).  S is a compile-time constant: S = 1 for the scene point cloud (n_half == 0: every
// projection lane of a round is a live (edge, pixel) pair), S = 8 for the point-flow hypotheses (7 of them in one segment); further
// segments are further workgroups.  The upstream gradient is channel-last, [n_ref * h * w, n_hyp, C]: the C lanes of a pixel read
// one contiguous row.
// The sample positions are the forward's, bit for bit: cam_block's K^-1 adjugate and rounded-product P = K [R|t] are the texts
// backproject.hip spells inline (compared term by term), the hypothesis depth is its add_rn(depth, (float)((double)(hyp - n_half) *
// offset)) -- i * offset evaluated in double, then rounded -- and world_point / sample_position are the same device functions.
// Float atomics: the order in which contributions reach a texel is not fixed, so the last bits of the feature gradient can differ
// from call to call.  The depth gradient is a second, small kernel, one thread per pixel, no atomics.
#include "variance_backward.h"

namespace {

using v3d::kCamStride;

struct BpBwdParams : v3d::VarianceBwdParams {       // n_samples = n_hyp, gvar [n_ref*h*w, n_hyp, C]
  const float* depth;         // [n_ref, h*w]
  const float* gpts;          // [n_ref*h*w, 1, 3]
  float* gdepth;              // [n_ref, h*w]
  int n_half;
  double offset;
  __device__ __forceinline__ float sample_depth(int r, int pixel, int hyp, bool live) const {
    return v3d::add_rn(live ? depth[(size_t)r * (h * w) + pixel] : 0.f, (float)((double)(hyp - n_half) * offset));
  }
  template <int C>
  __device__ __forceinline__ size_t gvar_index(int r, int pixel, int hyp, int c) const {
    return (((size_t)r * (h * w) + pixel) * n_samples + hyp) * C + c;
  }
};

template <int C, int S>
__global__ __launch_bounds__(64) void backproject_variance_backward_kernel(BpBwdParams p) {
  v3d::variance_backward_walk<C, S>(p);
}

// dL/ddepth of the scene point cloud, one thread per pixel: g = gP . ray, ray = R^T K^-1 (x, y, 1).  No atomics: repeated calls
// are bit-identical.  Orders (include/v3d.h): c_i = dot3_chain(Kinv[i,0], x, Kinv[i,1], y, Kinv[i,2], 1),
// ray_j = dot3_chain(R[0,j], c_0, R[1,j], c_1, R[2,j], c_2), g = dot3_chain(gP_0, ray_0, gP_1, ray_1, gP_2, ray_2).
__global__ __launch_bounds__(256) void backproject_depth_backward_kernel(BpBwdParams p) {
  __shared__ float s_cam[kCamStride];
  const int P = p.h * p.w;
  const int n_pt = (P + 255) / 256;
  const int r = (int)blockIdx.x / n_pt, pt = (int)blockIdx.x % n_pt;
  if (threadIdx.x == 0) {
    const int ref = p.ref_img[r];
    v3d::cam_block(p.K + ref * 9, p.R + ref * 9, p.t + ref * 3, s_cam);
  }
  __syncthreads();
  const int pix = pt * 256 + (int)threadIdx.x;
  if (pix >= P) return;
  const int gy = pix / p.w, gx = pix % p.w;
  const float x = v3d::psv_grid_coord(gx, p.w, p.W, p.x_step), y = v3d::psv_grid_coord(gy, p.h, p.H, p.y_step);
  const float c0 = v3d::dot3_chain(s_cam[0], x, s_cam[1], y, s_cam[2], 1.f);
  const float c1 = v3d::dot3_chain(s_cam[3], x, s_cam[4], y, s_cam[5], 1.f);
  const float c2 = v3d::dot3_chain(s_cam[6], x, s_cam[7], y, s_cam[8], 1.f);
  const float ray0 = v3d::dot3_chain(s_cam[9], c0, s_cam[12], c1, s_cam[15], c2);
  const float ray1 = v3d::dot3_chain(s_cam[10], c0, s_cam[13], c1, s_cam[16], c2);
  const float ray2 = v3d::dot3_chain(s_cam[11], c0, s_cam[14], c1, s_cam[17], c2);
  const size_t row = (size_t)r * P + pix;
  const float* gp = p.gpts + row * 3;
  p.gdepth[row] = v3d::dot3_chain(gp[0], ray0, gp[1], ray1, gp[2], ray2);
}

}  // namespace

extern "C" int v3d_backproject_variance_backward_f32(const float* depth, const float* feat_cl, const float* K, const float* R,
                                                     const float* t, const int32_t* ref_img, const int32_t* edge_ofs,
                                                     const int32_t* edge_src, int n_img, int n_ref, int n_edges, int C, int Hf,
                                                     int Wf, int H, int W, int h, int w, double offset, int n_half,
                                                     const float* grad_var, const float* grad_pts, float* grad_feat_cl,
                                                     float* grad_depth, void* stream) {
  const char* const fn = "v3d_backproject_variance_backward_f32";
  V3D_REQUIRE(depth && feat_cl && K && R && t && ref_img && edge_ofs && edge_src, V3D_ERR_BAD_ARG, "%s: null pointer argument", fn);
  V3D_REQUIRE((grad_var != nullptr) == (grad_feat_cl != nullptr), V3D_ERR_BAD_ARG,
              "%s: grad_var and grad_feat_cl go together (both or neither)", fn);
  V3D_REQUIRE((grad_pts != nullptr) == (grad_depth != nullptr), V3D_ERR_BAD_ARG,
              "%s: grad_pts and grad_depth go together (both or neither)", fn);
  V3D_REQUIRE(grad_var || grad_pts, V3D_ERR_BAD_ARG, "%s: neither gradient is asked for", fn);
  V3D_REQUIRE(!(grad_pts && n_half > 0), V3D_ERR_BAD_ARG,
              "%s: the hypothesis points (n_half > 0) are not differentiable with respect to the depth", fn);
  if (const int rc = v3d::variance_backward_limits(fn, n_img, n_ref, n_edges, C, Hf, Wf, H, W, h, w,
                                                   n_half >= 0 && n_half < (1 << 20)))
    return rc;
  V3D_REQUIRE((long long)h * w < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: depth map of 2^31 pixels or more", fn);

  BpBwdParams p;
  p.depth = depth; p.feat = feat_cl; p.K = K; p.R = R; p.t = t;
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src;
  p.gvar = grad_var; p.gpts = grad_pts; p.gfeat = grad_feat_cl; p.gdepth = grad_depth;
  p.n_half = n_half; p.offset = offset;
  const long long blocks = v3d::variance_backward_geometry(p, n_ref, C, Hf, Wf, H, W, h, w, 2 * n_half + 1, n_half == 0 ? 1 : 8);
  const long long dblocks = (long long)n_ref * (((long long)h * w + 255) / 256);
  V3D_REQUIRE(blocks < (1ll << 31) && dblocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: grid too large", fn);

  hipStream_t s = (hipStream_t)stream;
  if (grad_var) {
    V3D_CHECK_HIP(v3d::variance_backward_zero_fill(grad_feat_cl, n_img, Hf, Wf, C, s));
    {
      v3d::TimedScope ts("backproject_variance_backward", s);
      if (n_half == 0) {
        if (C == 32) backproject_variance_backward_kernel<32, 1><<<(unsigned)blocks, 64, 0, s>>>(p);
        else backproject_variance_backward_kernel<16, 1><<<(unsigned)blocks, 64, 0, s>>>(p);
      } else {
        if (C == 32) backproject_variance_backward_kernel<32, 8><<<(unsigned)blocks, 64, 0, s>>>(p);
        else backproject_variance_backward_kernel<16, 8><<<(unsigned)blocks, 64, 0, s>>>(p);
      }
    }
    V3D_CHECK_LAUNCH("backproject_variance_backward_kernel");
  }
  if (grad_pts) {
    {
      v3d::TimedScope ts("backproject_depth_backward", s);
      backproject_depth_backward_kernel<<<(unsigned)dblocks, 256, 0, s>>>(p);
    }
    V3D_CHECK_LAUNCH("backproject_depth_backward_kernel");
  }
  return V3D_OK;
}
