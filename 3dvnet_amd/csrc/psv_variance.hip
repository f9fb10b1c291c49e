// Rows A1-A4 of SURVEY.md §8a: plane-sweep homography warp of source-view features + cross-view variance, fused (no world
// points, sampling grid, warped volume or squared volume is ever materialised).  Reference semantics: mv3d/utils.py:86-108,
// mv3d/subnetworks/mvsnet.py:192-216.
//
// This file is the host side of the operation -- workspace plan, argument validation, the choice of the warp kernel and the
// extern "C" entry points -- and the map of its kernels, one unit per translation unit (psv_kernels.h declares what they share
// and their launchers; psv_common.h states the sample geometry, which the backward walk, variance_backward.h, shares):
//
//   psv_prepare.hip    feat [n_img, C, Hf, Wf] -> featT [n_img, Hf + 2, Wf + 2, C] (workspace): channel-last, so that one bilinear
//                      tap of all C channels is one contiguous run, with a border of zero cells, so that grid_sample's zero
//                      padding needs no test; K, R, t -> one camera block per image.  Also v3d_psv_sample_positions_f32, the
//                      diagnostic twin of the kernels' projection.
//   psv_window.hip     the window kernel, v3d_psv_kernel_choice() = 0: C = 32 and bordered maps below 2 GB, i.e. every product
//                      shape of the 32-channel network (44 % of path A).  A wave owns 8 pixels x 8 planes, copies
//                      the box its 64 footprints of an edge span into LDS and blends from there.  The only kernel that writes
//                      the cl8 layout; its tap words keep the sign bit as a flag, hence the 2 GB.
//   psv_fallback.hip   the reuse kernel, choice 1: C = 32 with bordered maps of 2 GB and more (32-bit byte offsets, < 4 GB), or
//                      the developer option psv_kernel = 1.  The same wave, footprints kept in registers from plane to plane.
//                      The gather kernel, choice 2: C = 16 (PL3DVNet's default feat_dim), or psv_kernel = 2.  Four taps
//                      gathered per (pixel, plane, edge); the only kernel templated on C.
//
// The three kernels sample at the same positions (psv_common.h), blend the taps and accumulate the views in the same order and
// share the epilogue arithmetic: their outputs agree bit for bit (tests/test_costvolume_gpu.py).
//   var    [n_ref, C, D, h, w] (reference layout, consumed as-is by the 3D-conv regulariser), or the split / cl8 hand-off
//          layouts of include/v3d.h.
#include "psv_kernels.h"

using v3d::kCamStride;
using v3d::PsvParams;

// bordered channel-last feature maps: n_img x (Hf + 2) x (Wf + 2) cells + the tail of zero cells behind them
static size_t psv_feat_bytes(int n_img, int C, int Hf, int Wf) {
  return ((size_t)n_img * (Hf + 2) * (Wf + 2) + v3d::kTailCells(Wf)) * C * sizeof(float);
}

extern "C" size_t v3d_psv_workspace_bytes(int n_img, int C, int Hf, int Wf) {
  // channel-last copy of the feature maps + the per-image camera blocks
  return v3d::align_up(psv_feat_bytes(n_img, C, Hf, Wf), 256) + v3d::align_up((size_t)n_img * kCamStride * sizeof(float), 256);
}

// The ONE statement of which warp kernel a call takes: the channel count, the developer option "psv_kernel" (0 auto, 1 reuse,
// 2 gather) and the size of the bordered maps -- the window kernel's tap words keep their sign bit as a flag, so maps of 2 GB
// and more take the reuse kernel.
enum { kPsvWindow = 0, kPsvReuse = 1, kPsvGather = 2 };
extern "C" int v3d_psv_kernel_choice(int n_img, int C, int Hf, int Wf) {
  V3D_REQUIRE(C == 32 || C == 16, V3D_ERR_UNSUPPORTED, "v3d_psv_kernel_choice: C=%d unsupported (16 or 32)", C);
  V3D_REQUIRE(n_img > 0 && Hf > 0 && Wf > 0, V3D_ERR_BAD_SHAPE, "v3d_psv_kernel_choice: bad shape");
  const int psv_kernel = v3d::option(v3d::kOptPsvKernel);
  if (C != 32 || psv_kernel == 2) return kPsvGather;
  if (psv_kernel == 1 || psv_feat_bytes(n_img, C, Hf, Wf) >= ((size_t)1 << 31)) return kPsvReuse;
  return kPsvWindow;
}

void v3d::psv_fill_grid(PsvParams& p, int H, int W, double depth_start, double depth_interval, int D, int h, int w) {
  p.H = H; p.W = W; p.D = D; p.h = h; p.w = w;
  p.x_step = w > 1 ? (double)(W - 1) / (double)(w - 1) : 0.0;
  p.y_step = h > 1 ? (double)(H - 1) / (double)(h - 1) : 0.0;
  const double depth_end = depth_start + (double)(D - 1) * depth_interval;
  p.z_start = depth_start;
  p.z_step = D > 1 ? (depth_end - depth_start) / (double)(D - 1) : 0.0;
  p.z_end = depth_end;
}

static int psv_variance_impl(int layout, const float* feat, const float* K, const float* R, const float* t, const int32_t* ref_img,
                             const int32_t* edge_ofs, const int32_t* edge_src, int n_img, int n_ref, int n_edges, int C, int Hf,
                             int Wf, int H, int W, double depth_start, double depth_interval, int D, int h, int w, float* var,
                             void* workspace, size_t workspace_bytes, void* stream) {
  const bool split = layout != V3D_LAYOUT_REFERENCE, cl8 = layout == V3D_LAYOUT_CL8;
  V3D_REQUIRE(feat && K && R && t && ref_img && edge_ofs && edge_src && var && workspace,
              V3D_ERR_BAD_ARG, "v3d_psv_variance_f32: null pointer argument");
  V3D_REQUIRE(C == 32 || C == 16, V3D_ERR_UNSUPPORTED,
              "v3d_psv_variance_f32: C=%d unsupported (16 or 32)", C);
  // the kernels divide by W - 1 and H - 1 through their correctly rounded reciprocals (exact unless the divisor's
  // significand is all ones, i.e. >= 2^24 - 1)
  V3D_REQUIRE(W <= (1 << 20) && H <= (1 << 20), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: image size out of range");
  V3D_REQUIRE(!split || C == 32, V3D_ERR_UNSUPPORTED,
              "v3d_psv_variance_split: C=%d unsupported (the split layout is defined for 32 channels)", C);
  V3D_REQUIRE(n_img > 0 && n_ref > 0 && n_edges >= 0 && Hf > 0 && Wf > 0 && H > 1 && W > 1 &&
                  D > 0 && h > 0 && w > 0,
              V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: bad shape");
  V3D_REQUIRE(Hf < 32760 && Wf < 32760, V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: feature maps larger than 32759 cells per axis");
  V3D_REQUIRE(psv_feat_bytes(n_img, C, Hf, Wf) < (size_t)1 << 32, V3D_ERR_BAD_SHAPE,
              "v3d_psv_variance_f32: bordered feature maps exceed 4 GB (32-bit byte offsets)");
  V3D_REQUIRE(workspace_bytes >= v3d_psv_workspace_bytes(n_img, C, Hf, Wf),
              V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_psv_variance_f32: workspace %zu < %zu",
              workspace_bytes, v3d_psv_workspace_bytes(n_img, C, Hf, Wf));
  const int choice = v3d_psv_kernel_choice(n_img, C, Hf, Wf);
  V3D_REQUIRE(!cl8 || choice != kPsvReuse, V3D_ERR_UNSUPPORTED,
              "v3d_psv_variance_cl8: only the window kernel writes this layout (feature maps < 2 GB, no developer switch)");
  V3D_REQUIRE(!cl8 || choice != kPsvGather, V3D_ERR_UNSUPPORTED,
              "v3d_psv_variance_cl8: C=%d unsupported (32) / option psv_kernel = 2", C);
  hipStream_t s = (hipStream_t)stream;
  float* featT = (float*)workspace;
  float* camp = (float*)((char*)workspace + v3d::align_up(psv_feat_bytes(n_img, C, Hf, Wf), 256));
  if (int rc = v3d::launch_psv_prepare(feat, K, R, t, n_img, C, Hf, Wf, featT, camp, s)) return rc;

  PsvParams p = {};
  p.featT = featT; p.K = K; p.R = R; p.t = t;
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src; p.var = var; p.camp = camp;
  p.n_img = n_img; p.n_ref = n_ref; p.Hf = Hf; p.Wf = Wf;
  v3d::psv_fill_grid(p, H, W, depth_start, depth_interval, D, h, w);
  v3d::TimedScope ts("psv_variance", s);
  return choice == kPsvWindow ? v3d::launch_psv_window(p, layout, s)
         : choice == kPsvReuse ? v3d::launch_psv_reuse(p, layout, s)
                               : v3d::launch_psv_gather(p, C, layout, s);
}

extern "C" int v3d_psv_variance_f32(const float* feat, const float* K, const float* R, const float* t,
                                    const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                    int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                    double depth_start, double depth_interval, int D, int h, int w, float* var,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return psv_variance_impl(V3D_LAYOUT_REFERENCE, feat, K, R, t, ref_img, edge_ofs, edge_src, n_img, n_ref, n_edges, C, Hf, Wf,
                           H, W, depth_start, depth_interval, D, h, w, var, workspace, workspace_bytes, stream);
}

extern "C" int v3d_psv_variance_split(const float* feat, const float* K, const float* R, const float* t,
                                      const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                      int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                      double depth_start, double depth_interval, int D, int h, int w,
                                      void* var_split, void* workspace, size_t workspace_bytes, void* stream) {
  return psv_variance_impl(V3D_LAYOUT_SPLIT, feat, K, R, t, ref_img, edge_ofs, edge_src, n_img, n_ref, n_edges, C, Hf, Wf, H, W,
                           depth_start, depth_interval, D, h, w, (float*)var_split, workspace, workspace_bytes, stream);
}

extern "C" int v3d_psv_variance_cl8(const float* feat, const float* K, const float* R, const float* t,
                                    const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                    int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                    double depth_start, double depth_interval, int D, int h, int w,
                                    float* var_cl8, void* workspace, size_t workspace_bytes, void* stream) {
  return psv_variance_impl(V3D_LAYOUT_CL8, feat, K, R, t, ref_img, edge_ofs, edge_src, n_img, n_ref, n_edges, C, Hf, Wf, H, W,
                           depth_start, depth_interval, D, h, w, var_cl8, workspace, workspace_bytes, stream);
}
