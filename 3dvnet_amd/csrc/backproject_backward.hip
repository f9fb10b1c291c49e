// Backward of the back-projected variance (rows B1-B2 / C1; backproject.hip is the forward): v3d_backproject_variance_backward_f32,
// include/v3d.h.  Reference semantics: the autograd of mv3d/lightningmodel.py:132-174 (construct_feature_rich_pointcloud) and
// :187-235 (run_pointflow).  The reference builds the sampling grid under torch.no_grad() in both, so exactly two gradients exist:
//
//   var -> features (n_half >= 0).  Per reference view r with cnt edges, per pixel, hypothesis and channel:  x_e = bilinear sample
//     of source e (zeros padding), avg = sum_e x_e / cnt, var = sum_e x_e^2 / cnt - avg^2.  Given gV = dL/dvar:
//         g_e = gV * 2 * (x_e - avg) / cnt          dL/dfeat[src_e, tap, c] += w_tap * g_e   for the in-image taps.
//   pts -> depth (n_half == 0 only).  pts = R^T (K^-1 (p d) - t), p = (x, y, 1):  dL/dd = sum_j gP_j ray_j,  ray = R^T K^-1 p.
//
// The feature kernel is psv_backward.hip's with the hypothesis axis in the place of the plane axis: single-wave workgroups, one per
// (reference view, 64 / C pixels, segment of S hypotheses); lane = (pixel, channel), so the C lanes of a pixel read and add one
// contiguous 4 C-byte texel.
//   projection  one lane per (edge, hypothesis, pixel): footprint cell, validity of its four taps, weights -> LDS records;
//   pass 1      every lane walks its pixel's hypotheses for every edge: sum of x_e -> avg (S registers);
//   pass 2      the same walk again, edge by edge: g_e, and the four tap sums of the CURRENT footprint stay in registers; they are
//               flushed (up to four atomic adds) only when the footprint moves to another cell -- at an offset of 0.05 m consecutive
//               hypotheses of a pixel move a fraction of a quarter-resolution texel.
// More than 8 edges per view go through LDS in chunks of 8 and are projected again in pass 2.  S is a compile-time constant: S = 1
// for the scene point cloud (n_half == 0: every projection lane of a round is a live (edge, pixel) pair), S = 8 for the
// point-flow hypotheses (7 of them in one segment); further segments are further workgroups.
// The sample positions are the forward's, bit for bit: cam_block's K^-1 adjugate and rounded-product P = K [R|t] are the texts
// backproject.hip spells inline (compared term by term), the hypothesis depth is its add_rn(depth, (float)((double)(hyp - n_half) *
// offset)), and world_point / sample_position are the same device functions.  psv_footprint's clamp gives the forward's "outside:
// nothing is sampled" -- a NaN or out-of-range position has no valid tap with a non-zero weight.
// Float atomics: the order in which contributions reach a texel is not fixed, so the last bits of the feature gradient can differ
// from call to call.  The depth gradient is a second, small kernel, one thread per pixel, no atomics.
#include "psv_common.h"

namespace {

using v3d::kCamStride;

constexpr int kBMaxE = 8;     // edges per LDS pass

struct BpBwdParams {
  const float* depth;         // [n_ref, h*w]
  const float* feat;          // [n_img, Hf, Wf, C]
  const float* K;
  const float* R;
  const float* t;
  const int* ref_img;
  const int* edge_ofs;
  const int* edge_src;
  const float* gvar;          // [n_ref*h*w, n_hyp, C]
  const float* gpts;          // [n_ref*h*w, 1, 3]
  float* gfeat;               // [n_img, Hf, Wf, C], zero-filled before the launch
  float* gdepth;              // [n_ref, h*w]
  int Hf, Wf, H, W, h, w, n_hyp, n_half, n_ptile, n_seg;
  double x_step, y_step, offset;
};

// One (edge, hypothesis, pixel) sample, 32 bytes: psv_backward.hip's record.  The four cells are addressed through CLAMPED
// coordinates (always inside the source image); a tap outside the image carries weight 0 (it adds nothing to x_e) and no
// validity bit (it receives no gradient).
struct BwdTap {
  float w00, w01, w10, w11;   // nw, ne, sw, se
  unsigned row0, row1;        // first cell of the (clamped) upper / lower row of the footprint, counted over all images
  unsigned xx;                // clamped left column | clamped right column << 16
  unsigned key;               // footprint identity: nw cell of the bordered grid ((y0 + 1) (Wf + 2) + x0 + 1) | validity << 28
};
constexpr unsigned kNoKey = 0x0fffffffu;      // no footprint: validity 0, a cell number no image has (host check)

template <int C, int S>
__global__ __launch_bounds__(64) void backproject_variance_backward_kernel(BpBwdParams p) {
  constexpr int PPW = 64 / C;               // pixels per wave
  constexpr int ITEMS = PPW * S;            // (hypothesis, pixel) samples per edge
  constexpr int EPR = 64 / ITEMS;           // edges projected per round
  static_assert(PPW >= 1 && EPR >= 1 && EPR * ITEMS == 64, "lane roles");
  __shared__ BwdTap s_tap[kBMaxE * ITEMS];
  __shared__ float s_cam[1 + kBMaxE][kCamStride];      // [0] the reference view, [1 + e] the chunk's source views

  const int lane = threadIdx.x;
  const int c = lane % C, px = lane / C;
  int b = v3d::xcd_contiguous_block();
  const int seg = b % p.n_seg; b /= p.n_seg;            // hypothesis segments fastest
  const int ptile = b % p.n_ptile;
  const int r = b / p.n_ptile;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], ne = p.edge_ofs[r + 1] - e_begin;
  if (ne == 0) return;                                  // a view without edges: var == 0 whatever the features are (wave-uniform)
  const int ref = p.ref_img[r];
  const int hyp0 = seg * S;

  // projection role: lane = (edge slot, hypothesis, pixel)
  const int item = lane % ITEMS, e1 = lane / ITEMS, hy1 = item / PPW, px1 = item % PPW;
  const int gp1 = ptile * PPW + px1, hyp1 = hyp0 + hy1;
  const bool live1 = gp1 < P && hyp1 < p.n_hyp;
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  const float rWm1 = (float)(1.0 / (double)(p.W - 1)), rHm1 = (float)(1.0 / (double)(p.H - 1));
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);
  float X = 0.f, Y = 0.f, Z = 0.f;

  // camera blocks of the chunk's source views (and, with the first chunk, of the reference view), one lane per image
  auto load_cams = [&](int ec, int nec) __attribute__((always_inline)) {
    if (lane <= nec && (lane > 0 || ec == 0)) {
      const int img = lane == 0 ? ref : p.edge_src[e_begin + ec + lane - 1];
      v3d::cam_block(p.K + img * 9, p.R + img * 9, p.t + img * 3, s_cam[lane]);
    }
  };
  auto project = [&](int ec, int nec) __attribute__((always_inline)) {
    for (int e = e1; e < nec; e += EPR) {
      float ix, iy;
      v3d::sample_position(s_cam[1 + e] + 24, X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
      const v3d::Footprint f = v3d::psv_footprint(ix, iy, p.Wf, p.Hf);
      const int x0 = (int)f.x0, y0 = (int)f.y0;          // in [-1, Wf] x [-1, Hf]
      const bool vx0 = x0 >= 0 && x0 < p.Wf, vx1 = x0 + 1 < p.Wf, vy0 = y0 >= 0 && y0 < p.Hf, vy1 = y0 + 1 < p.Hf;
      const unsigned valid = live1 ? (unsigned)(vx0 && vy0) | (unsigned)(vx1 && vy0) << 1 | (unsigned)(vx0 && vy1) << 2 |
                                         (unsigned)(vx1 && vy1) << 3
                                   : 0u;
      const int x0c = min(max(x0, 0), p.Wf - 1), x1c = min(x0 + 1, p.Wf - 1);
      const int y0c = min(max(y0, 0), p.Hf - 1), y1c = min(y0 + 1, p.Hf - 1);
      const unsigned img_row = (unsigned)p.edge_src[e_begin + ec + e] * (unsigned)p.Hf;
      BwdTap ti;
      ti.w00 = (valid & 1u) ? f.w00 : 0.f; ti.w01 = (valid & 2u) ? f.w01 : 0.f;
      ti.w10 = (valid & 4u) ? f.w10 : 0.f; ti.w11 = (valid & 8u) ? f.w11 : 0.f;
      ti.row0 = (img_row + (unsigned)y0c) * (unsigned)p.Wf;
      ti.row1 = (img_row + (unsigned)y1c) * (unsigned)p.Wf;
      ti.xx = (unsigned)x0c | (unsigned)x1c << 16;
      ti.key = (unsigned)((y0 + 1) * (p.Wf + 2) + x0 + 1) | valid << 28;
      s_tap[e * ITEMS + item] = ti;
    }
  };
  // the four cells of a footprint, this lane's channel: kept in registers while the walk stays in one footprint
  struct Cells { float v00, v01, v10, v11; };
  auto gather = [&](const BwdTap& ti) __attribute__((always_inline)) {
    const unsigned x0c = ti.xx & 0xffffu, x1c = ti.xx >> 16;
    return Cells{p.feat[(size_t)(ti.row0 + x0c) * C + c], p.feat[(size_t)(ti.row0 + x1c) * C + c],
                 p.feat[(size_t)(ti.row1 + x0c) * C + c], p.feat[(size_t)(ti.row1 + x1c) * C + c]};
  };
  // x_e: F.grid_sample's tap order as an FMA chain, as in the forward kernel
  auto blend = [&](const Cells& v, const BwdTap& ti) __attribute__((always_inline)) {
    float s = v3d::mul_rn(v.v00, ti.w00);
    s = __builtin_fmaf(v.v01, ti.w01, s);
    s = __builtin_fmaf(v.v10, ti.w10, s);
    return __builtin_fmaf(v.v11, ti.w11, s);
  };

  // ---- pass 1: sum of the samples over the edges, per hypothesis -----------------------------------------------
  float avg[S];
#pragma unroll
  for (int k = 0; k < S; ++k) avg[k] = 0.f;
  for (int ec = 0; ec < ne; ec += kBMaxE) {
    const int nec = min(kBMaxE, ne - ec);
    __syncthreads();                       // the previous chunk's records and camera blocks are read
    load_cams(ec, nec);
    __syncthreads();
    if (ec == 0) {
      const int gy = gp1 / p.w, gx = gp1 % p.w;
      // the forward's hypothesis depth: depth + i * offset with i * offset evaluated in double, then rounded
      const float dep = v3d::add_rn(live1 ? p.depth[(size_t)r * P + gp1] : 0.f, (float)((double)(hyp1 - p.n_half) * p.offset));
      v3d::world_point(s_cam[0], v3d::psv_grid_coord(gx, p.w, p.W, p.x_step), v3d::psv_grid_coord(gy, p.h, p.H, p.y_step), dep,
                       X, Y, Z);
    }
    project(ec, nec);
    __syncthreads();
    for (int e = 0; e < nec; ++e) {
      unsigned key = kNoKey;
      Cells v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const BwdTap ti = s_tap[e * ITEMS + k * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          v = gather(ti);
          key = ti.key;
        }
        avg[k] = v3d::add_rn(avg[k], blend(v, ti));
        asm volatile("" : "+v"(avg[k]) : : "memory");    // one hypothesis after the other (see psv_backward.hip)
      }
    }
  }

  // ---- avg, and gV * 2 / cnt of this lane's samples ------------------------------------------------------------
  const float cnt = (float)ne;
  const float two_over_cnt = 2.f / cnt;
  const int gp = ptile * PPW + px;
  float gs[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    avg[k] = avg[k] / cnt;
    const int hyp = hyp0 + k;
    // channel-last: the C lanes of a pixel read one contiguous row
    gs[k] = (gp < P && hyp < p.n_hyp) ? v3d::mul_rn(p.gvar[(((size_t)r * P + gp) * p.n_hyp + hyp) * C + c], two_over_cnt) : 0.f;
  }

  // ---- pass 2: g_e, tap sums of the current footprint in registers, atomic adds when the footprint moves ----
  const bool one_chunk = ne <= kBMaxE;     // the records of pass 1 are still in LDS
  for (int ec = 0; ec < ne; ec += kBMaxE) {
    const int nec = min(kBMaxE, ne - ec);
    if (!one_chunk) {
      __syncthreads();
      load_cams(ec, nec);
      __syncthreads();
      project(ec, nec);
      __syncthreads();
    }
    for (int e = 0; e < nec; ++e) {
      unsigned key = kNoKey, row0 = 0, row1 = 0, xx = 0;
      float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;
      auto flush = [&]() __attribute__((always_inline)) {
        const unsigned x0c = xx & 0xffffu, x1c = xx >> 16;
        if (key & (1u << 28)) atomicAdd(p.gfeat + (size_t)(row0 + x0c) * C + c, a00);
        if (key & (2u << 28)) atomicAdd(p.gfeat + (size_t)(row0 + x1c) * C + c, a01);
        if (key & (4u << 28)) atomicAdd(p.gfeat + (size_t)(row1 + x0c) * C + c, a10);
        if (key & (8u << 28)) atomicAdd(p.gfeat + (size_t)(row1 + x1c) * C + c, a11);
      };
      Cells v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const BwdTap ti = s_tap[e * ITEMS + k * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          flush();
          key = ti.key; row0 = ti.row0; row1 = ti.row1; xx = ti.xx;
          a00 = a01 = a10 = a11 = 0.f;
          v = gather(ti);
        }
        const float g = v3d::mul_rn(v3d::sub_rn(blend(v, ti), avg[k]), gs[k]);
        a00 = __builtin_fmaf(ti.w00, g, a00);
        a01 = __builtin_fmaf(ti.w01, g, a01);
        a10 = __builtin_fmaf(ti.w10, g, a10);
        a11 = __builtin_fmaf(ti.w11, g, a11);
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11) : : "memory");
      }
      flush();
    }
  }
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
  V3D_REQUIRE(C == 32 || C == 16, V3D_ERR_UNSUPPORTED, "%s: C=%d unsupported (16 or 32)", fn, C);
  V3D_REQUIRE(W <= (1 << 20) && H <= (1 << 20), V3D_ERR_BAD_SHAPE, "%s: image size out of range", fn);
  V3D_REQUIRE(n_img > 0 && n_ref > 0 && n_edges >= 0 && Hf > 0 && Wf > 0 && H > 1 && W > 1 && h > 0 && w > 0 && n_half >= 0 &&
                  n_half < (1 << 20),
              V3D_ERR_BAD_SHAPE, "%s: bad shape", fn);
  // tap records: 16-bit columns, 28-bit cell numbers of the bordered grid, 32-bit cell and element numbers over all images
  V3D_REQUIRE(Hf < 32760 && Wf < 32760 && (long long)(Hf + 2) * (Wf + 2) < (long long)kNoKey, V3D_ERR_BAD_SHAPE,
              "%s: feature maps too large (32759 cells per axis, 2^28 per image)", fn);
  V3D_REQUIRE((long long)n_img * Hf * Wf * C < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: feature stack of 2^31 elements or more", fn);
  V3D_REQUIRE((long long)h * w < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: depth map of 2^31 pixels or more", fn);

  BpBwdParams p;
  p.depth = depth; p.feat = feat_cl; p.K = K; p.R = R; p.t = t;
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src;
  p.gvar = grad_var; p.gpts = grad_pts; p.gfeat = grad_feat_cl; p.gdepth = grad_depth;
  p.Hf = Hf; p.Wf = Wf; p.H = H; p.W = W; p.h = h; p.w = w;
  p.n_hyp = 2 * n_half + 1; p.n_half = n_half; p.offset = offset;
  const int seg_len = n_half == 0 ? 1 : 8;
  const int ppw = 64 / C;
  p.n_ptile = (int)(((long long)h * w + ppw - 1) / ppw);
  p.n_seg = (p.n_hyp + seg_len - 1) / seg_len;
  p.x_step = w > 1 ? (double)(W - 1) / (double)(w - 1) : 0.0;
  p.y_step = h > 1 ? (double)(H - 1) / (double)(h - 1) : 0.0;
  const long long blocks = (long long)n_ref * p.n_ptile * p.n_seg;
  const long long dblocks = (long long)n_ref * (((long long)h * w + 255) / 256);
  V3D_REQUIRE(blocks < (1ll << 31) && dblocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: grid too large", fn);

  hipStream_t s = (hipStream_t)stream;
  if (grad_var) {
    // output contract: the entry point zero-fills its accumulation target itself
    V3D_CHECK_HIP(hipMemsetAsync(grad_feat_cl, 0, (size_t)n_img * Hf * Wf * C * sizeof(float), s));
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
