// Backward of the fused plane-sweep warp + variance (rows A1-A4; psv_variance.hip is the map of the forward) with respect to the features
// (v3d_psv_variance_backward_f32, include/v3d.h).  Reference semantics: the autograd of mvsnet.py:209-216.
//
// Per reference view r with cnt edges, per channel and voxel:  x_e = bilinear sample of source e (zeros padding),
// avg = sum_e x_e / cnt, var = sum_e x_e^2 / cnt - avg^2.  Given gV = dL/dvar:
//     g_e = gV * 2 * (x_e - avg) / cnt          dL/dfeat[src_e, tap, c] += w_tap * g_e   for the in-image taps.
// Cameras and plane depths are data.  Like the forward, nothing of size E * C * D * h * w exists: the samples are taken
// again from the channel-last features.  No scratch memory either: every workgroup forms the camera blocks it needs in its
// prologue (psv_common.h: cam_block, the arithmetic of the forward's cam_setup_kernel) and the accumulation target is the
// output itself.  The sample positions are the forward's, bit for bit: world_point / sample_position / psv_footprint are
// the same device functions.
//
// Work decomposition: one single-wave workgroup per (reference view, 64 / C plane-grid pixels, segment of kBDS planes).
// Lane = (pixel, channel): the C lanes of a pixel read and add one contiguous 4 C-byte texel -- with C = 32 an atomic
// wave-instruction is two 128-byte texel rows, the shape global float atomics run at full rate with.
//   projection  one lane per (edge, plane, pixel): footprint cell, validity of its four taps, weights -> LDS records;
//   pass 1      every lane walks its pixel's planes for every edge: sum of x_e -> avg (kBDS registers);
//   pass 2      the same walk again, edge by edge: g_e, and the four tap sums of the CURRENT footprint stay in registers;
//               they are flushed (up to four atomic adds) only when the footprint moves to another cell -- at far planes a
//               sample moves a fraction of a texel per plane, so consecutive planes share their footprint.
//   In both passes the four cells of the current footprint stay in registers as well and are gathered again only when the
//   footprint moves.
// Float atomics: the order in which contributions reach a texel is not fixed, so the last bits of the gradient can differ
// from call to call.
#include "psv_common.h"

namespace {

using v3d::kCamStride;

constexpr int kBDS = 16;      // depth planes a wave walks (one depth segment)
constexpr int kBMaxE = 8;     // edges per LDS pass

struct PsvBwdParams {
  const float* feat;          // [n_img, Hf, Wf, C]
  const float* K;
  const float* R;
  const float* t;
  const int* ref_img;
  const int* edge_ofs;
  const int* edge_src;
  const float* gvar;          // [n_ref, C, D, h, w]
  float* gfeat;               // [n_img, Hf, Wf, C], zero-filled before the launch
  int Hf, Wf, H, W, D, h, w, n_ptile, n_dseg;
  double x_step, y_step, z_start, z_step, z_end;
};

// One (edge, plane, pixel) sample, 32 bytes.  The four cells are addressed through CLAMPED coordinates (always inside the
// source image); a tap outside the image carries weight 0 here (it adds nothing to x_e) and no validity bit (it receives
// no gradient).
struct BwdTap {
  float w00, w01, w10, w11;   // nw, ne, sw, se
  unsigned row0, row1;        // first cell of the (clamped) upper / lower row of the footprint, counted over all images
  unsigned xx;                // clamped left column | clamped right column << 16
  unsigned key;               // footprint identity: nw cell of the bordered grid ((y0 + 1) (Wf + 2) + x0 + 1) | validity << 28
};
constexpr unsigned kNoKey = 0x0fffffffu;      // no footprint: validity 0, a cell number no image has (host check)

template <int C>
__global__ __launch_bounds__(64) void psv_variance_backward_kernel(PsvBwdParams p) {
  constexpr int PPW = 64 / C;               // pixels per wave
  constexpr int ITEMS = PPW * kBDS;         // (plane, pixel) samples per edge
  constexpr int EPR = 64 / ITEMS;           // edges projected per round
  static_assert(PPW >= 1 && EPR >= 1 && EPR * ITEMS == 64, "lane roles");
  __shared__ BwdTap s_tap[kBMaxE * ITEMS];
  __shared__ float s_cam[1 + kBMaxE][kCamStride];      // [0] the reference view, [1 + e] the chunk's source views

  const int lane = threadIdx.x;
  const int c = lane % C, px = lane / C;
  int b = v3d::xcd_contiguous_block();
  const int dseg = b % p.n_dseg; b /= p.n_dseg;         // depth segments fastest (see psv_fallback.hip, the reuse kernel)
  const int ptile = b % p.n_ptile;
  const int r = b / p.n_ptile;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], ne = p.edge_ofs[r + 1] - e_begin;
  const int ref = p.ref_img[r];
  const int d0 = dseg * kBDS;

  // projection role: lane = (edge slot, plane, pixel)
  const int item = lane % ITEMS, e1 = lane / ITEMS, pl1 = item / PPW, px1 = item % PPW;
  const int gp1 = ptile * PPW + px1, d1 = d0 + pl1;
  const bool live1 = gp1 < P && d1 < p.D;
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
  // The four cells of a footprint, this lane's channel.  Both passes keep them in registers while the walk along the depth axis
  // stays in one footprint and load them again only when it moves on (as the forward's plane-reuse kernel does): the
  // vector-memory path is charged per wave INSTRUCTION, and four 4-byte gathers per sample were what bounded
  // this kernel -- on 4 of 5 planes the footprint is the previous plane's.
  struct Cells { float v00, v01, v10, v11; };
  auto gather = [&](const BwdTap& ti) __attribute__((always_inline)) {
    const unsigned x0c = ti.xx & 0xffffu, x1c = ti.xx >> 16;
    return Cells{p.feat[(size_t)(ti.row0 + x0c) * C + c], p.feat[(size_t)(ti.row0 + x1c) * C + c],
                 p.feat[(size_t)(ti.row1 + x0c) * C + c], p.feat[(size_t)(ti.row1 + x1c) * C + c]};
  };
  // x_e: F.grid_sample's tap order as an FMA chain, as in the forward kernels
  auto blend = [&](const Cells& v, const BwdTap& ti) __attribute__((always_inline)) {
    float s = v3d::mul_rn(v.v00, ti.w00);
    s = __builtin_fmaf(v.v01, ti.w01, s);
    s = __builtin_fmaf(v.v10, ti.w10, s);
    return __builtin_fmaf(v.v11, ti.w11, s);
  };

  // ---- pass 1: sum of the samples over the edges, per plane ---------------------------------------------------
  float avg[kBDS];
#pragma unroll
  for (int pl = 0; pl < kBDS; ++pl) avg[pl] = 0.f;
  for (int ec = 0; ec < ne; ec += kBMaxE) {
    const int nec = min(kBMaxE, ne - ec);
    __syncthreads();                       // the previous chunk's records and camera blocks are read
    load_cams(ec, nec);
    __syncthreads();
    if (ec == 0) {
      const int gy = gp1 / p.w, gx = gp1 % p.w;
      v3d::world_point(s_cam[0], v3d::psv_grid_coord(gx, p.w, p.W, p.x_step), v3d::psv_grid_coord(gy, p.h, p.H, p.y_step),
                       v3d::psv_plane_depth(d1, p.D, p.z_start, p.z_step, p.z_end), X, Y, Z);
    }
    project(ec, nec);
    __syncthreads();
    for (int e = 0; e < nec; ++e) {
      unsigned key = kNoKey;
      Cells v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int pl = 0; pl < kBDS; ++pl) {
        const BwdTap ti = s_tap[e * ITEMS + pl * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          v = gather(ti);
          key = ti.key;
        }
        avg[pl] = v3d::add_rn(avg[pl], blend(v, ti));
        // Finish this plane before the next one starts: the empty statement pins the sum here and, as a memory barrier, keeps
        // the next plane's record read and gather below it (the compiler otherwise reads the records of all kBDS planes
        // first and blends last, 12 registers per plane: 182 VGPRs, 2 waves per SIMD)
        asm volatile("" : "+v"(avg[pl]) : : "memory");
      }
    }
  }
  if (ne == 0) return;                     // a view without edges: var == 0 whatever the features are

  // ---- avg, and gV * 2 / cnt of this lane's voxels ------------------------------------------------------------
  const float cnt = (float)ne;
  const float two_over_cnt = 2.f / cnt;
  const int gp = ptile * PPW + px;
  float gs[kBDS];
#pragma unroll
  for (int pl = 0; pl < kBDS; ++pl) {
    avg[pl] = avg[pl] / cnt;
    const int d = d0 + pl;
    gs[pl] = (gp < P && d < p.D) ? v3d::mul_rn(p.gvar[(((size_t)r * C + c) * p.D + d) * P + gp], two_over_cnt) : 0.f;
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
      for (int pl = 0; pl < kBDS; ++pl) {
        const BwdTap ti = s_tap[e * ITEMS + pl * PPW + px];
        if (ti.key != key) {               // the same for the C lanes of a pixel
          flush();
          key = ti.key; row0 = ti.row0; row1 = ti.row1; xx = ti.xx;
          a00 = a01 = a10 = a11 = 0.f;
          v = gather(ti);
        }
        const float g = v3d::mul_rn(v3d::sub_rn(blend(v, ti), avg[pl]), gs[pl]);
        a00 = __builtin_fmaf(ti.w00, g, a00);
        a01 = __builtin_fmaf(ti.w01, g, a01);
        a10 = __builtin_fmaf(ti.w10, g, a10);
        a11 = __builtin_fmaf(ti.w11, g, a11);
        asm volatile("" : "+v"(a00), "+v"(a01), "+v"(a10), "+v"(a11) : : "memory");   // one plane after the other, as in pass 1
      }
      flush();
    }
  }
}

}  // namespace

extern "C" int v3d_psv_variance_backward_f32(const float* feat_cl, const float* K, const float* R, const float* t,
                                             const int32_t* ref_img, const int32_t* edge_ofs, const int32_t* edge_src,
                                             int n_img, int n_ref, int n_edges, int C, int Hf, int Wf, int H, int W,
                                             double depth_start, double depth_interval, int D, int h, int w,
                                             const float* grad_var, float* grad_feat_cl, void* stream) {
  V3D_REQUIRE(feat_cl && K && R && t && ref_img && edge_ofs && edge_src && grad_var && grad_feat_cl, V3D_ERR_BAD_ARG,
              "v3d_psv_variance_backward_f32: null pointer argument");
  V3D_REQUIRE(C == 32 || C == 16, V3D_ERR_UNSUPPORTED, "v3d_psv_variance_backward_f32: C=%d unsupported (16 or 32)", C);
  V3D_REQUIRE(W <= (1 << 20) && H <= (1 << 20), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_backward_f32: image size out of range");
  V3D_REQUIRE(n_img > 0 && n_ref > 0 && n_edges >= 0 && Hf > 0 && Wf > 0 && H > 1 && W > 1 && D > 0 && h > 0 && w > 0,
              V3D_ERR_BAD_SHAPE, "v3d_psv_variance_backward_f32: bad shape");
  // tap records: 16-bit columns, 28-bit cell numbers of the bordered grid, 32-bit cell and element numbers over all images
  V3D_REQUIRE(Hf < 32760 && Wf < 32760 && (long long)(Hf + 2) * (Wf + 2) < (long long)kNoKey, V3D_ERR_BAD_SHAPE,
              "v3d_psv_variance_backward_f32: feature maps too large (32759 cells per axis, 2^28 per image)");
  V3D_REQUIRE((long long)n_img * Hf * Wf * C < (1ll << 31), V3D_ERR_BAD_SHAPE,
              "v3d_psv_variance_backward_f32: feature stack of 2^31 elements or more");
  hipStream_t s = (hipStream_t)stream;
  // output contract: the entry point zero-fills its accumulation target itself
  V3D_CHECK_HIP(hipMemsetAsync(grad_feat_cl, 0, (size_t)n_img * Hf * Wf * C * sizeof(float), s));

  PsvBwdParams p;
  p.feat = feat_cl; p.K = K; p.R = R; p.t = t;
  p.ref_img = ref_img; p.edge_ofs = edge_ofs; p.edge_src = edge_src; p.gvar = grad_var; p.gfeat = grad_feat_cl;
  p.Hf = Hf; p.Wf = Wf; p.H = H; p.W = W; p.D = D; p.h = h; p.w = w;
  const int ppw = 64 / C;
  p.n_ptile = (h * w + ppw - 1) / ppw;
  p.n_dseg = (D + kBDS - 1) / kBDS;
  p.x_step = w > 1 ? (double)(W - 1) / (double)(w - 1) : 0.0;
  p.y_step = h > 1 ? (double)(H - 1) / (double)(h - 1) : 0.0;
  const double depth_end = depth_start + (double)(D - 1) * depth_interval;
  p.z_start = depth_start;
  p.z_step = D > 1 ? (depth_end - depth_start) / (double)(D - 1) : 0.0;
  p.z_end = depth_end;
  const long long blocks = (long long)n_ref * p.n_ptile * p.n_dseg;
  V3D_REQUIRE(blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_backward_f32: grid too large");
  {
    v3d::TimedScope ts("psv_variance_backward", s);
    if (C == 32) psv_variance_backward_kernel<32><<<(unsigned)blocks, 64, 0, s>>>(p);
    else psv_variance_backward_kernel<16><<<(unsigned)blocks, 64, 0, s>>>(p);
  }
  V3D_CHECK_LAUNCH("psv_variance_backward_kernel");
  return V3D_OK;
}
