// Rows A5-A6 of SURVEY.md §8a: CostRegNet (dense 3D-conv U-Net, eval-mode BatchNorm folded) and the
// soft-argmin depth.  Reference semantics: mv3d/subnetworks/mvsnet.py:18-36,133-163,219-227.
//
// This file is the host side of the regulariser -- the weight handle, the workspace plan, the two chains and the extern "C"
// entry points -- and the map of its kernels, one family per translation unit (costreg.h declares their launchers and packers):
//
// (1) The fused path (v3d_costreg_depth_f32 / _split): every layer on split-bf16 matrix cores.  Each fp32 operand
//     x = hi + lo (hi = RNE_bf16(x), lo = RNE_bf16(x - hi), 16 mantissa bits), each product hi*hi + hi*lo + lo*hi on
//     v_mfma_f32_16x16x32_bf16 with fp32 accumulation; activations travel between layers in the split channel-last
//     layout [n][C/8 groups][hi, lo][D][H][W][8 bf16] (4 bytes per value, every staging loop a 16-byte copy):
//       conv0z.hip           conv0, 32 -> 8 at full resolution (68 % of the MACs), as a depth march
//       conv12z.hip          conv1 + conv2 as one depth march
//       costreg_convg.hip    convg_bf16x2_kernel: conv1..conv6 (stride 1 / 2), 8 input channels per chunk, 16 output channels per
//                            workgroup; deconvg_bf16x2_kernel: conv7, conv8 (transposed conv as a GEMM over 2x2x2 output cells)
//                            + skip; encode_split_kernel: fp32 -> the split layout
//       costreg_conv9.hip    conv9_prob_kernel: conv9 + conv0 skip + the 8 -> 1 prob conv, the 8-channel tensor stays in LDS
//       confidence.hip       soft_argmin_kernel: softmax(-x) expectation over the depth planes, alone or with the confidence
//     Final depth vs the fp32 CPU oracle: 5e-5 relative (gate 1e-4).
//
// (2) The exact-fp32 path (v3d_costreg_layer_f32, and the whole chain with precision = V3D_PRECISION_FP32):
//       costreg_fp32.hip     conv3d_mfma_kernel: one templated implicit-GEMM kernel on v_mfma_f32_16x16x4_f32 per layer
//       conv0z.hip           conv0 of the chain on the fp32 channel-last volume (v3d_costreg_depth_cl8)
//       costreg_conv9.hip    conv9 + skip + prob on the exact-fp32 variant of conv9_prob_kernel
//
// (3) The per-layer entry points of the split kernels (parity tests against (2)): costreg_conv0.hip (conv0_bf16x2_kernel, fp32 in
//     and out) behind v3d_costreg_layer_f32 with V3D_PRECISION_SPLIT_BF16, costreg_convg.hip behind v3d_costreg_layer_split_f32.
#include <cstdlib>
#include <vector>

#include "costreg.h"
#include "weight_pack.h"

using v3d::kLayers;
using v3d::kOutF32;
using v3d::kOutSplit;

extern "C" int v3d_costreg_pack(const float* const* conv_w, const float* const* bn_w,
                                const float* const* bn_b, const float* const* bn_m,
                                const float* const* bn_v, const float* prob_w, const float* prob_b,
                                int in_channels, int base, float eps,
                                v3d_costreg_weights** out_handle) {
  V3D_REQUIRE(conv_w && bn_w && bn_b && bn_m && bn_v && prob_w && prob_b && out_handle,
              V3D_ERR_BAD_ARG, "v3d_costreg_pack: null argument");
  V3D_REQUIRE((in_channels == 32 || in_channels == 16) && base == 8, V3D_ERR_UNSUPPORTED,
              "v3d_costreg_pack: CostRegNet(32, 8) and CostRegNet(16, 8) are built (got %d, %d)", in_channels, base);
  v3d_costreg_weights* h = new v3d_costreg_weights();
  h->in_channels = in_channels; h->base = base;
  v3d::HostImage img;
  std::vector<float> wf[10];      // BN-folded weights of every layer, in the layout of conv_w[l]
  for (int l = 0; l < 10; ++l) {
    const int cin = l == 0 ? in_channels : kLayers[l].cin, cout = kLayers[l].cout;
    const v3d::BnFold bn(bn_w[l], bn_b[l], bn_m[l], bn_v[l], eps, cout);
    wf[l] = kLayers[l].deconv ? bn.weights(conv_w[l], cin, 27) : bn.weights(conv_w[l], 1, (size_t)cin * 27);
    h->wp_ofs[l] = img.reserve(v3d::tile_image_floats(l, in_channels));
    h->bias_ofs[l] = img.reserve(cout);
    v3d::pack_tile_image(l, in_channels, wf[l].data(), img.at(h->wp_ofs[l]));
    memcpy(img.at(h->bias_ofs[l]), bn.bias.data(), cout * sizeof(float));
  }
  h->c0bf_ofs = img.reserve(v3d::kConv0SplitFloats);
  v3d::pack_conv0_split(wf[0].data(), in_channels, img.words(h->c0bf_ofs));
  h->c0f32_ofs = img.reserve(v3d::kConv0F32Floats);
  v3d::pack_conv0_f32(wf[0].data(), in_channels, img.at(h->c0f32_ofs));
  h->c9bf_ofs = img.reserve(v3d::kConv9SplitFloats);
  h->c9f32_ofs = img.reserve(v3d::kConv9F32Floats);
  v3d::pack_conv9(wf[9].data(), img.words(h->c9bf_ofs), img.at(h->c9f32_ofs));
  for (int l = 1; l <= 8; ++l) {
    const int cin = kLayers[l].cin, cout = kLayers[l].cout;
    size_t& ofs = l <= 6 ? h->cgbf_ofs[l] : h->dgbf_ofs[l - 7];
    ofs = img.reserve((size_t)(cout / 16) * (cin / 8) * (l <= 6 ? 9 : 12) * 2 * v3d::kLoWords);
    if (l <= 6) v3d::pack_convg(wf[l].data(), cin, cout, img.words(ofs));
    else v3d::pack_deconvg(wf[l].data(), cin, cout, img.words(ofs));
  }
  h->prob_w2_ofs = img.reserve((size_t)base * 27);
  v3d::pack_prob(prob_w, img.at(h->prob_w2_ofs));
  h->prob_b_ofs = img.reserve(1);
  *img.at(h->prob_b_ofs) = prob_b[0];
  h->total = img.data.size();
  return v3d::finish_pack(h, img.data.data(), h->total * sizeof(float), "weights", out_handle);
}

extern "C" void v3d_costreg_free(v3d_costreg_weights* h) { v3d::release(h); }

// One layer on fp32 [n, C, D, H, W] tensors: the exact-fp32 kernels, or (conv0 only) the split-bf16 tile kernel
static int run_layer(const v3d_costreg_weights* h, int layer, const float* in, const float* skip,
                     float* out, int n, int Di, int Hi, int Wi, int precision, hipStream_t s) {
  const float* wp = h->dev + h->wp_ofs[layer];
  const float* bias = h->dev + h->bias_ofs[layer];
  if (layer == 0 && precision != V3D_PRECISION_FP32) {
    V3D_REQUIRE(h->in_channels != 16, V3D_ERR_UNSUPPORTED,
                "costreg: the per-layer conv0 of CostRegNet(16, 8) is built for V3D_PRECISION_FP32 only (the chain entry points "
                "cover both precisions)");
    return v3d::launch_conv0_bf16(in, h->dev + h->c0bf_ofs, bias, skip, out, n, Di, Hi, Wi, s);
  }
  return v3d::launch_conv_fp32(layer, h->in_channels, in, wp, bias, skip, out, n, Di, Hi, Wi, s);
}

extern "C" int v3d_costreg_layer_f32(const v3d_costreg_weights* h, int layer, const float* in,
                                     const float* skip, int n, int Di, int Hi, int Wi, float* out,
                                     int precision, void* stream) {
  V3D_REQUIRE(h && in && out, V3D_ERR_BAD_ARG, "v3d_costreg_layer_f32: null argument");
  V3D_REQUIRE(n > 0 && Di > 0 && Hi > 0 && Wi > 0, V3D_ERR_BAD_SHAPE, "v3d_costreg_layer_f32: bad shape");
  V3D_REQUIRE(precision == V3D_PRECISION_SPLIT_BF16 || precision == V3D_PRECISION_FP32, V3D_ERR_BAD_ARG,
              "v3d_costreg_layer_f32: unknown precision %d", precision);
  return run_layer(h, layer, in, skip, out, n, Di, Hi, Wi, precision, (hipStream_t)stream);
}

extern "C" size_t v3d_costreg_layer_split_workspace_bytes(int n, int cin, int Di, int Hi, int Wi) {
  if (n <= 0 || cin <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0) return 0;
  return v3d::align_up((size_t)n * cin * Di * Hi * Wi * sizeof(float), 256);
}

extern "C" int v3d_costreg_layer_split_f32(const v3d_costreg_weights* h, int layer, const float* in, const float* skip,
                                           int n, int Di, int Hi, int Wi, float* out, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(h && in && out && workspace, V3D_ERR_BAD_ARG, "v3d_costreg_layer_split_f32: null argument");
  V3D_REQUIRE(layer >= 1 && layer <= 8, V3D_ERR_BAD_ARG, "v3d_costreg_layer_split_f32: layer %d (1..8: conv1..conv8)", layer);
  V3D_REQUIRE(n > 0 && Di > 0 && Hi > 0 && Wi > 0, V3D_ERR_BAD_SHAPE, "v3d_costreg_layer_split_f32: bad shape");
  V3D_REQUIRE(layer < 7 || skip, V3D_ERR_BAD_ARG, "v3d_costreg_layer_split_f32: conv7 / conv8 need the skip tensor");
  const int cin = kLayers[layer].cin;
  V3D_REQUIRE(workspace_bytes >= v3d_costreg_layer_split_workspace_bytes(n, cin, Di, Hi, Wi), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_costreg_layer_split_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const size_t plane = (size_t)Di * Hi * Wi, total = (size_t)n * (cin / 8) * plane;
  if (const int rc = v3d::launch_encode_split(in, workspace, cin, plane, total, s); rc != V3D_OK) return rc;
  const float* w = h->dev + (layer <= 6 ? h->cgbf_ofs[layer] : h->dgbf_ofs[layer - 7]);
  return v3d::launch_split_layer(layer, kOutF32, workspace, w, h->dev + h->bias_ofs[layer], skip, out, n, Di, Hi, Wi, s);
}

namespace {
struct WsPlan { size_t c0, c1, c2, c3, c4, c5, c6, u7, u8, u9, reg, enc, total; };
WsPlan plan_ws(int n, int D, int h, int w) {
  const size_t V0 = (size_t)D * h * w, V1 = V0 / 8, V2 = V1 / 8, V3 = V2 / 8;
  WsPlan p; size_t o = 0;
  auto take = [&](size_t nf) { size_t r = o; o += v3d::align_up(nf * sizeof(float), 256); return r; };
  p.c0 = take(n * 8 * V0); p.c1 = take(n * 16 * V1); p.c2 = take(n * 16 * V1);
  p.c3 = take(n * 32 * V2); p.c4 = take(n * 32 * V2); p.c5 = take(n * 64 * V3);
  p.c6 = take(n * 64 * V3); p.u7 = take(n * 32 * V2); p.u8 = take(n * 16 * V1);
  p.u9 = take(n * 8 * V0); p.reg = take(n * V0);
  p.enc = take(32 * V0);        // ONE view's variance volume in the split layout (fp32 entry point, see costreg_depth_impl)
  p.total = o;
  return p;
}
}  // namespace

extern "C" size_t v3d_costreg_workspace_bytes(const v3d_costreg_weights*, int n_ref, int D, int h, int w) {
  if (n_ref <= 0 || D <= 0 || h <= 0 || w <= 0) return 0;
  return plan_ws(n_ref, D, h, w).total;
}

namespace {
// The optional confidence output of the depth entry points (v3d_costreg_depth_prob): with `prob` set, the last launch is the
// soft-argmin that also writes the confidence (confidence.hip: same depth bits); without it, soft_argmin_kernel as ever.
struct ProbOut {
  float* prob = nullptr;
  double depth_start = 0., depth_interval = 0.;
};

int launch_depth_tail(const float* xreg, const float* depth_vals, float* depth, const ProbOut& po, int n, int D, int H, int W,
                      hipStream_t s) {
  if (!po.prob) return v3d::launch_soft_argmin(xreg, depth_vals, depth, n, D, H, W, s);
  return v3d::launch_soft_argmin_prob(xreg, depth_vals, depth, po.prob, po.depth_start, po.depth_interval, n, D, H, W, s);
}

// The split-bf16 regulariser behind conv0, on the caller's stream: conv1 + conv2, conv3 .. conv8, conv9 + skip + prob,
// soft-argmin.
int run_split_tail(const v3d_costreg_weights* h, const WsPlan& ws, char* base, const float* depth_vals, int n, int D, int H, int W,
                   float* depth, float* xreg, const ProbOut& po, hipStream_t s) {
  const size_t V1 = (size_t)D * H * W / 8;
  auto F = [&](size_t o) { return (float*)(base + o); };
  // conv1..conv6 hand their activations on in the split layout; the transposed convolutions read their skips (conv2, conv4)
  // from the same split copies (DG::SKIP_SPLIT).  The split copies live in the u9 slot of the workspace, which the fused
  // conv9+prob kernel does not need.
  float* const c2s = F(ws.u9);
  float* const c4s = c2s + (size_t)n * 16 * V1;
  auto W_ = [&](int l) { return h->dev + h->cgbf_ofs[l]; };
  auto B_ = [&](int l) { return h->dev + h->bias_ofs[l]; };
  // conv1..conv8 of the chain: split layout in and out, the skips (conv2, conv4) in the split layout as well
  auto L_ = [&](int l, const float* in, const float* skip, float* out, int d, int hh, int ww) {
    return v3d::launch_split_layer(l, kOutSplit, in, l <= 6 ? W_(l) : h->dev + h->dgbf_ofs[l - 7], B_(l), skip, out, n, d, hh, ww, s);
  };
#ifdef V3D_PHASE_TIMING
  const int stop_after = v3d::option(v3d::kOptStopAfter);   // isolate one kernel's counters
#else
  const int stop_after = 99;
#endif
  int rc = V3D_OK;
  if (stop_after < 1) return rc;
  // conv1 + conv2: the fused depth march of conv12z.hip (conv1's output never leaves LDS: 0.27 ms per 64 cfg2 views against
  // 0.176 + 0.146 for the two tile kernels, which remain behind the developer option c12_march = 0 and the per-layer entry points)
  if (v3d::option(v3d::kOptC12March) != 0) {
    rc = v3d::launch_conv12z(F(ws.c0), W_(1), W_(2), B_(1), B_(2), c2s, n, D, H, W, s);
  } else if ((rc = L_(1, F(ws.c0), nullptr, F(ws.c1), D, H, W)) == V3D_OK) {
    rc = L_(2, F(ws.c1), nullptr, c2s, D / 2, H / 2, W / 2);
  }
  if (rc != V3D_OK || stop_after < 3) return rc;
  if ((rc = L_(3, c2s, nullptr, F(ws.c3), D / 2, H / 2, W / 2)) != V3D_OK || stop_after < 4) return rc;
  if ((rc = L_(4, F(ws.c3), nullptr, c4s, D / 4, H / 4, W / 4)) != V3D_OK || stop_after < 5) return rc;
  if ((rc = L_(5, c4s, nullptr, F(ws.c5), D / 4, H / 4, W / 4)) != V3D_OK || stop_after < 6) return rc;
  if ((rc = L_(6, F(ws.c5), nullptr, F(ws.c6), D / 8, H / 8, W / 8)) != V3D_OK || stop_after < 7) return rc;
  if ((rc = L_(7, F(ws.c6), c4s, F(ws.u7), D / 8, H / 8, W / 8)) != V3D_OK || stop_after < 8) return rc;     // conv4 + conv7(x) (mvsnet.py:159)
  if ((rc = L_(8, F(ws.u7), c2s, F(ws.u8), D / 4, H / 4, W / 4)) != V3D_OK || stop_after < 9) return rc;     // conv2 + conv8(x) (:160)
  if ((rc = v3d::launch_conv9_prob(false, h, F(ws.u8), F(ws.c0), xreg, n, D, H, W, s)) != V3D_OK || stop_after < 10) return rc;
  return launch_depth_tail(xreg, depth_vals, depth, po, n, D, H, W, s);
}
}  // namespace

// in_layout: 0 = reference fp32 [n, C, D, h, w], 1 = split-bf16 hand-off, 2 = fp32 channel-last (v3d_psv_variance_cl8)
static int costreg_depth_impl(int in_layout, const v3d_costreg_weights* h, const float* var,
                              const float* depth_vals, int n, int D, int H, int W,
                              float* depth, float* reg, int precision, void* workspace,
                              size_t workspace_bytes, void* stream, const ProbOut& po = ProbOut()) {
  V3D_REQUIRE(precision == V3D_PRECISION_SPLIT_BF16 || precision == V3D_PRECISION_FP32, V3D_ERR_BAD_ARG,
              "v3d_costreg_depth_f32: unknown precision %d", precision);
  V3D_REQUIRE(h && var && depth_vals && depth && workspace, V3D_ERR_BAD_ARG,
              "v3d_costreg_depth_f32: null argument");
  V3D_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && D % 8 == 0 && H % 8 == 0 && W % 8 == 0,
              V3D_ERR_BAD_SHAPE, "v3d_costreg_depth_f32: D,h,w must be positive multiples of 8 (got %d,%d,%d)", D, H, W);
  const WsPlan ws = plan_ws(n, D, H, W);
  V3D_REQUIRE(workspace_bytes >= ws.total, V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_costreg_depth_f32: workspace %zu < %zu", workspace_bytes, ws.total);
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  auto F = [&](size_t o) { return (float*)(base + o); };
  float* xreg = reg ? reg : F(ws.reg);
  int rc;
#define RUN(layer, in, skip, out, d, hh, ww) \
  if ((rc = run_layer(h, layer, in, skip, out, n, d, hh, ww, V3D_PRECISION_FP32, s)) != V3D_OK) return rc;
  // precision == V3D_PRECISION_FP32 (fp32 volume only): every layer on the exact-fp32 per-layer kernels with fp32
  // [n, C, D, H, W] tensors in between.  V3D_PRECISION_SPLIT_BF16: every layer on split-bf16 matrix cores, activations
  // in the split channel-last hand-off format (same bytes as fp32).
  const bool generic = precision == V3D_PRECISION_FP32;
  const bool split_in = in_layout == 1, cl8_in = in_layout == 2;
  V3D_REQUIRE(!generic || !split_in, V3D_ERR_UNSUPPORTED, "V3D_PRECISION_FP32 needs an fp32 variance volume");
  V3D_REQUIRE(h->in_channels == 32 || in_layout == 0, V3D_ERR_UNSUPPORTED,
              "CostRegNet(16, 8) takes the variance volume in the reference layout (the hand-off formats are defined for 32 channels)");
  V3D_REQUIRE(generic || !cl8_in, V3D_ERR_UNSUPPORTED, "the fp32 channel-last volume is the input of V3D_PRECISION_FP32");
  if (generic) {
    if (cl8_in) {      // conv0 as a depth march on exact-fp32 matrix instructions (conv0z.hip)
      if ((rc = v3d::launch_conv0z(true, var, h->dev + h->c0f32_ofs, h->dev + h->bias_ofs[0], F(ws.c0), n, D, H, W, s)) != V3D_OK)
        return rc;
    } else {
      RUN(0, var, nullptr, F(ws.c0), D, H, W);
    }
    RUN(1, F(ws.c0), nullptr, F(ws.c1), D, H, W);
    RUN(2, F(ws.c1), nullptr, F(ws.c2), D / 2, H / 2, W / 2);
  } else {
    // conv0: the depth-march kernel (conv0z.hip) reads the split hand-off format.  The fp32 entry point (CostRegNet.forward
    // on a reference-layout tensor, return_intermediates) encodes one view at a time into the workspace's `enc` slot and runs
    // the same kernel on it: both entry points give the same bits.
    if (split_in) {
      if ((rc = v3d::launch_conv0z(false, var, h->dev + h->c0bf_ofs, h->dev + h->bias_ofs[0], F(ws.c0), n, D, H, W, s)) != V3D_OK) return rc;
    } else {
      // (CostRegNet(16, 8): channel groups 2, 3 of the encoded view are zeros, once -- their conv0 weights are zero as well)
      const int cin = h->in_channels, ngrp = cin / 8;
      const size_t V0 = (size_t)D * H * W, total = (size_t)ngrp * V0;
      if (ngrp < 4) V3D_CHECK_HIP(hipMemsetAsync((char*)F(ws.enc) + (size_t)ngrp * 2 * V0 * 16, 0, (size_t)(4 - ngrp) * 2 * V0 * 16, s));
      for (int i = 0; i < n; ++i) {
        if ((rc = v3d::launch_encode_split(var + (size_t)i * cin * V0, F(ws.enc), cin, V0, total, s)) != V3D_OK) return rc;
        if ((rc = v3d::launch_conv0z(false, F(ws.enc), h->dev + h->c0bf_ofs, h->dev + h->bias_ofs[0], F(ws.c0) + (size_t)i * 8 * V0, 1, D, H,
                                     W, s)) != V3D_OK) return rc;
      }
    }
    // conv1 .. conv9 + prob, soft-argmin
    return run_split_tail(h, ws, base, depth_vals, n, D, H, W, depth, xreg, po, s);
  }
  RUN(3, F(ws.c2), nullptr, F(ws.c3), D / 2, H / 2, W / 2);
  RUN(4, F(ws.c3), nullptr, F(ws.c4), D / 4, H / 4, W / 4);
  RUN(5, F(ws.c4), nullptr, F(ws.c5), D / 4, H / 4, W / 4);
  RUN(6, F(ws.c5), nullptr, F(ws.c6), D / 8, H / 8, W / 8);
  RUN(7, F(ws.c6), F(ws.c4), F(ws.u7), D / 8, H / 8, W / 8);    // conv4 + conv7(x)  (mvsnet.py:159)
  RUN(8, F(ws.u7), F(ws.c2), F(ws.u8), D / 4, H / 4, W / 4);    // conv2 + conv8(x)  (:160)
  // conv9 + skip + prob on exact-fp32 operands: the tile kernel
  if ((rc = v3d::launch_conv9_prob(true, h, F(ws.u8), F(ws.c0), xreg, n, D, H, W, s)) != V3D_OK) return rc;
#undef RUN
  return launch_depth_tail(xreg, depth_vals, depth, po, n, D, H, W, s);
}

extern "C" int v3d_costreg_depth_f32(const v3d_costreg_weights* h, const float* var, const float* depth_vals, int n,
                                     int D, int H, int W, float* depth, float* reg, int precision, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return costreg_depth_impl(0, h, var, depth_vals, n, D, H, W, depth, reg, precision, workspace, workspace_bytes,
                            stream);
}

extern "C" int v3d_costreg_depth_cl8(const v3d_costreg_weights* h, const void* var_cl8, const float* depth_vals,
                                     int n, int D, int H, int W, float* depth, float* reg, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return costreg_depth_impl(2, h, (const float*)var_cl8, depth_vals, n, D, H, W, depth, reg, V3D_PRECISION_FP32, workspace,
                            workspace_bytes, stream);
}

extern "C" int v3d_costreg_depth_split(const v3d_costreg_weights* h, const void* var_split, const float* depth_vals,
                                       int n, int D, int H, int W, float* depth, float* reg, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return costreg_depth_impl(1, h, (const float*)var_split, depth_vals, n, D, H, W, depth, reg,
                            V3D_PRECISION_SPLIT_BF16, workspace, workspace_bytes, stream);
}

// The chain of the three entry points above, the layout and the precision as arguments, and the confidence of the depth beside
// it (include/v3d.h).  Everything is validated before the first launch.
extern "C" int v3d_costreg_depth_prob(const v3d_costreg_weights* h, const void* var, int in_layout, int precision,
                                      const float* depth_vals, double depth_start, double depth_interval, int n, int D, int H,
                                      int W, float* depth, float* reg, float* prob, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  V3D_REQUIRE(in_layout == V3D_LAYOUT_REFERENCE || in_layout == V3D_LAYOUT_SPLIT || in_layout == V3D_LAYOUT_CL8, V3D_ERR_BAD_ARG,
              "v3d_costreg_depth_prob: unknown input layout %d", in_layout);
  const float ds = (float)depth_start, di = (float)depth_interval;
  V3D_REQUIRE(std::isfinite(ds) && std::isfinite(di) && di != 0.f, V3D_ERR_BAD_ARG,
              "v3d_costreg_depth_prob: depth_start = %g / depth_interval = %g must be finite fp32 numbers, the interval not zero",
              depth_start, depth_interval);
  V3D_REQUIRE(D < (1 << 24), V3D_ERR_BAD_SHAPE, "v3d_costreg_depth_prob: D = %d too large", D);
  ProbOut po;
  po.prob = prob; po.depth_start = depth_start; po.depth_interval = depth_interval;
  return costreg_depth_impl(in_layout, h, (const float*)var, depth_vals, n, D, H, W, depth, reg, precision, workspace,
                            workspace_bytes, stream, po);
}

// The last kernel of the chain alone, on a volume the caller holds: soft_argmin_kernel (prob == NULL) or the soft-argmin that also
// writes the confidence.  Any D, h, w.
extern "C" int v3d_soft_argmin_f32(const float* x_reg, const float* depth_vals, double depth_start, double depth_interval, int n,
                                   int D, int H, int W, float* depth, float* prob, void* stream) {
  V3D_REQUIRE(x_reg && depth_vals && depth, V3D_ERR_BAD_ARG, "v3d_soft_argmin_f32: null argument");
  V3D_REQUIRE(n > 0 && D > 0 && H > 0 && W > 0 && D < (1 << 24) && (long long)H * W < (1ll << 31) &&
                  ((long long)n * H * W + 255) / 256 < (1ll << 31),
              V3D_ERR_BAD_SHAPE, "v3d_soft_argmin_f32: n, D, h, w = %d, %d, %d, %d", n, D, H, W);
  const float ds = (float)depth_start, di = (float)depth_interval;
  V3D_REQUIRE(!prob || (std::isfinite(ds) && std::isfinite(di) && di != 0.f), V3D_ERR_BAD_ARG,
              "v3d_soft_argmin_f32: depth_start = %g / depth_interval = %g must be finite fp32 numbers, the interval not zero",
              depth_start, depth_interval);
  ProbOut po;
  po.prob = prob; po.depth_start = depth_start; po.depth_interval = depth_interval;
  return launch_depth_tail(x_reg, depth_vals, depth, po, n, D, H, W, (hipStream_t)stream);
}
