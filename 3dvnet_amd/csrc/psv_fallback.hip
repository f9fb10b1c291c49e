// Plane-sweep warp + variance: the two kernels behind the window kernel (psv_variance.hip is the map of the family and says
// which shapes they serve).  Both write what the window kernel writes, bit for bit: the same geometry (psv_common.h), the same
// tap order and accumulation order per (pixel, plane), the same epilogue (psv_kernels.h).
#include "psv_kernels.h"

namespace v3d {
namespace {

// ---------------------------------------------------------------------------------------------------
// Gather kernel (C = 16 or 32).  feat [n_img, C, Hf, Wf] arrives as featT [n_img, Hf + 2, Wf + 2, C] (psv_prepare.hip), so
// that one bilinear tap of all C channels is one contiguous 4*C-byte run (C = 32: exactly one 128-B cache line).
// One single-wave workgroup per (reference view, chunk of kGDB depth planes, tile of kGPix plane-grid pixels).  Per plane:
//   phase 1  every (pixel, edge) pair is projected once (results in LDS): the tap record of make_taps;
//   phase 2  C/4 lanes per pixel; each lane gathers float4 (4 channels) for the 4 taps of every edge -- the C/4 lanes of a
//            pixel read one full contiguous run per tap -- and accumulates sum / sum of squares in registers in edge order
//            (deterministic);
//   phase 3  the [C][kGPix] tile is transposed through LDS and written as rows of `var`.
// The phases of a workgroup are separated by barriers; with single-wave workgroups the barriers are free and the 24 resident
// waves of a CU drift apart, so the L1 (the binding resource, busy only during the gather phase) always has some wave gathering.
constexpr int kGThreads = 64;
constexpr int kGPix = 16;     // plane-grid pixels per workgroup
constexpr int kGDB = 4;       // depth planes per workgroup

template <int C, bool SPLIT>
__global__ __launch_bounds__(kGThreads) void psv_variance_kernel(PsvParams p) {
  constexpr int LP = C / 4;               // lanes per pixel
  constexpr int PPP = kGThreads / LP;     // pixels per phase-2 pass
  constexpr int NPASS = kGPix / PPP;
  static_assert(kGPix % PPP == 0, "tile");

  __shared__ TapInfo s_tap[kMaxE * kGPix];
  __shared__ __attribute__((aligned(16))) float s_out[C][kGPix + 1];
  __shared__ float s_ref[24];             // Kinv(9) R(9) t(3)
  __shared__ float s_P[kMaxE][12];

  const int tid = threadIdx.x;
  const int n_dchunk = (p.D + kGDB - 1) / kGDB;
  // every XCD takes a contiguous run of reference views, so its L2 holds the source feature maps of one
  // reference (~E x 400 KB) instead of all 8 dies streaming the sources of every reference in flight
  int b = xcd_contiguous_block();
  const int ptile = b % p.n_ptile; b /= p.n_ptile;
  const int dchunk = b % n_dchunk;
  const int r = b / n_dchunk;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], e_end = p.edge_ofs[r + 1];
  const int ne = e_end - e_begin;
  const int ref = p.ref_img[r];

  // K^-1 (9), R (9), t (3) of the reference view, prepared by cam_setup_kernel
  if (tid < 21) s_ref[tid] = p.camp[ref * kCamStride + tid];

  // this thread's phase-2 role
  const int cg = tid % LP;
  const int pix_in_pass = tid / LP;

  // pixel coordinates of this thread's phase-1 pixel (same pixel for every pair it handles)
  const int px1 = tid % kGPix;
  const int gp1 = ptile * kGPix + px1;
  const float xf = psv_grid_coord(gp1 % p.w, p.w, p.W, p.x_step), yf = psv_grid_coord(gp1 / p.w, p.h, p.H, p.y_step);
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  const float rWm1 = (float)(1.0 / (double)(p.W - 1)), rHm1 = (float)(1.0 / (double)(p.H - 1));
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);

  for (int dd = 0; dd < kGDB; ++dd) {
    const int d = dchunk * kGDB + dd;
    if (d >= p.D) break;
    const float z = psv_plane_depth(d, p.D, p.z_start, p.z_step, p.z_end);
    f32x4 acc_s[NPASS], acc_q[NPASS];
#pragma unroll
    for (int a = 0; a < NPASS; ++a) acc_s[a] = acc_q[a] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ec = 0; ec < ne; ec += kMaxE) {
      const int nec = min(kMaxE, ne - ec);
      __syncthreads();   // previous users of s_tap / s_P / s_out are done; s_ref visible
      // projection matrices P = K [R|t] of this chunk's source views (mvsnet.py:196-197); with a single chunk
      // of edges (the usual case) they are the same for every plane of the workgroup: computed once
      if (dd == 0 || ne > kMaxE) {
        for (int i = tid; i < nec * 12; i += kGThreads)
          s_P[i / 12][i % 12] = p.camp[p.edge_src[e_begin + ec + i / 12] * kCamStride + 24 + i % 12];
      }
      __syncthreads();
      // ---- phase 1: project (pixel, edge) pairs ------------------------------------------
      {
        float X, Y, Z;
        world_point(s_ref, xf, yf, z, X, Y, Z);
        for (int e = tid / kGPix; e < nec; e += kGThreads / kGPix) {
          float ix, iy;
          sample_position(s_P[e], X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
          s_tap[e * kGPix + px1] = make_taps<4 * C>(ix, iy, p.Wf, p.Hf, p.edge_src[e_begin + ec + e] * (p.Hf + 2) * (p.Wf + 2));
        }
      }
      __syncthreads();
      // ---- phase 2: gather + accumulate ----------------------------------------------------
#pragma unroll
      for (int a = 0; a < NPASS; ++a) {
        const int px = a * PPP + pix_in_pass;
        for (int e = 0; e < nec; ++e) {
          const TapInfo ti = s_tap[e * kGPix + px];
          // uniform base + 32-bit byte offset: the load takes the address as SGPR pair + VGPR offset
          const char* fb = reinterpret_cast<const char*>(p.featT);
          const unsigned cgb = cg * 16, rowb = (unsigned)(p.Wf + 2) * (4 * C);
          const f32x4 v00 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + cgb));
          const f32x4 v01 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + cgb) + 4 * C);
          const f32x4 v10 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + rowb + cgb));
          const f32x4 v11 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + rowb + cgb) + 4 * C);
          psv_blend_accumulate(v00, v01, v10, v11, ti, acc_s[a], acc_q[a]);
        }
      }
    }
    // ---- phase 3: variance, transpose through LDS, coalesced store ----------------------------
    const float cnt = (float)max(ne, 1);        // torch_scatter mean: sum / clamp(count, 1)
    auto mean = [&](float x) __attribute__((always_inline)) { return x / cnt; };
    if constexpr (SPLIT) {
      static_assert(!SPLIT || C == 32, "split layout is defined for 32 channels");
      // s_out reused as [8 groups][kGPix + 1] 16-byte slots (the +1 keeps the 4 channel groups off one bank).  The halves of a
      // slot meet in LDS, value by value with the scalar bf16_rne: not psv_split_slot's packed conversion, which differs from
      // it on NaN
      u32x2* const s_sp = reinterpret_cast<u32x2*>(&s_out[0][0]);
      const int chunk = cg >> 1, half = cg & 1;
#pragma unroll
      for (int a = 0; a < NPASS; ++a) {
        const int px = a * PPP + pix_in_pass;
        unsigned h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = psv_variance_value(acc_s[a][k], acc_q[a][k], mean);
          h[k] = bf16_rne(v);
          l[k] = bf16_rne(v - __uint_as_float(h[k] << 16));
        }
        s_sp[(((chunk * 2 + 0) * (kGPix + 1)) + px) * 2 + half] = (u32x2){h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        s_sp[(((chunk * 2 + 1) * (kGPix + 1)) + px) * 2 + half] = (u32x2){l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
      }
      __syncthreads();
      u32x4* const out = reinterpret_cast<u32x4*>(p.var);
      const u32x4* const s_q = reinterpret_cast<const u32x4*>(s_sp);
      for (int i = tid; i < 8 * kGPix; i += kGThreads) {
        const int g = i / kGPix, px = i % kGPix;
        const int gp = ptile * kGPix + px;
        if (gp < P) __builtin_nontemporal_store(s_q[g * (kGPix + 1) + px], &out[(((size_t)r * 8 + g) * p.D + d) * P + gp]);
      }
    } else {
#pragma unroll
      for (int a = 0; a < NPASS; ++a) {
        const int px = a * PPP + pix_in_pass;
#pragma unroll
        for (int k = 0; k < 4; ++k) s_out[cg * 4 + k][px] = psv_variance_value(acc_s[a][k], acc_q[a][k], mean);
      }
      __syncthreads();
      const int px = tid % kGPix, gp = ptile * kGPix + px;
      if (gp < P) {
        for (int c = tid / kGPix; c < C; c += kGThreads / kGPix)
          __builtin_nontemporal_store(s_out[c][px], &p.var[(((size_t)r * C + c) * p.D + d) * P + gp]);
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------------
// Plane-reuse kernel (C == 32).  The gather kernel above is bound by L1 bytes: 4 taps x 128 B per (pixel, plane, source
// view).  But the samples of one pixel on consecutive planes walk along its epipolar line in sub-pixel steps on most of the
// depth range, so their 2x2 footprints coincide (cfg2: the 16 taps of 4 consecutive planes touch 5.1 distinct cells on
// average).  Here a wave owns kRPix pixels x kRDB planes and projects one edge per pass, one (pixel, plane) sample per lane;
// the 8 lanes of a pixel keep the footprint of the previous plane in registers and reload it only when the footprint of the
// next plane differs.  Arithmetic and accumulation order per (pixel, plane) are those of the gather kernel (bit-identical
// output).
//
// What bounds it (DESIGN.md 4.1 has the round-2 measurements): no single pipe.  A footprint reload is four 1 KB wave loads,
// issued when ANY of the 8 pixels changed its footprint, with the other pixels' lanes masked: 1.8 wave loads per (plane, edge)
// step at 8 planes per wave (scripts/sim_footprint_reloads.py), although only 4 waves per SIMD fit.
//
// SPLIT = true: single-wave workgroups, the variance leaves in the regulariser's split format (16-byte slots, 128-byte runs per
// wave).  SPLIT = false (the public fp32 tensor [n_ref, C, D, h, w]): FOUR waves = four consecutive 8-pixel tiles per workgroup;
// they work independently and only share the output staging, so that a (channel, plane) row leaves as 32 consecutive pixels =
// 128-byte runs.  With one wave per workgroup the rows were 32-byte runs: 3.95 GB written for a 2.47 GB volume, 3.6 ms per 64
// views against 1.7 ms for the split variant.
template <bool SPLIT>
__global__ __launch_bounds__(SPLIT ? 64 : 256, V3D_PSV_WAVES) void psv_variance_reuse_kernel(PsvParams p) {
  constexpr int C = 32, WPB = SPLIT ? 1 : 4;
  constexpr int kOutPl = 4;               // planes staged per round of the fp32 epilogue
  static_assert(kRDB * kRPix == 64, "one (pixel, plane) sample per lane");
  static_assert(SPLIT || kRDB % kOutPl == 0, "fp32 epilogue stages 4 planes per round");
  __shared__ TapInfo s_tap_[WPB][kRDB * kRPix];
  __shared__ __attribute__((aligned(16))) float s_out[SPLIT ? 1 : kOutPl][SPLIT ? 1 : C][SPLIT ? 1 : WPB * kRPix + 1];
  __shared__ float s_ref_[WPB][24];
  __shared__ float s_P_[WPB][kMaxE][12];  // projection matrices of up to kMaxE consecutive edges
  __shared__ int s_base_[WPB][kMaxE];     // first feature cell of their source images

  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  TapInfo* const s_tap = s_tap_[wv];
  float* const s_ref = s_ref_[wv];
  float (*const s_P)[12] = s_P_[wv];
  int* const s_base = s_base_[wv];
  const int n_dchunk = (p.D + kRDB - 1) / kRDB;
  int b = xcd_contiguous_block();
  // plane chunks fastest: the waves resident on an XCD sweep all planes of a few pixel tiles, i.e. short epipolar segments of
  // the source maps, instead of one plane chunk of the whole image (= every source map entirely, more than the 4 MB L2)
  const int dchunk = b % n_dchunk; b /= n_dchunk;
  const int ptile = (b % p.n_ptile) * WPB + wv;      // p.n_ptile counts groups of WPB tiles
  const int r = b / p.n_ptile;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], e_end = p.edge_ofs[r + 1];
  const int ne = e_end - e_begin;
  const int ref = p.ref_img[r];
  if (lane < 21) s_ref[lane] = p.camp[ref * kCamStride + lane];
  psv_wave_sync<WPB>();

  // projection role: lane = (plane, pixel); the world point of (pixel, plane) is the same for every edge
  const int pl1 = lane >> 3, px1 = lane & 7;
  const int gp1 = ptile * kRPix + px1;
  const int d1 = dchunk * kRDB + pl1;
  float X, Y, Z;
  world_point(s_ref, psv_grid_coord(gp1 % p.w, p.w, p.W, p.x_step), psv_grid_coord(gp1 / p.w, p.h, p.H, p.y_step),
              psv_plane_depth(d1, p.D, p.z_start, p.z_step, p.z_end), X, Y, Z);
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  // divisions by the wave-uniform image extents go through their correctly rounded reciprocals (v3d::div_uniform)
  const float rWm1 = (float)(1.0 / (double)(p.W - 1)), rHm1 = (float)(1.0 / (double)(p.H - 1));
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);

  // gather role: 8 lanes x float4 per pixel
  const int gpx = lane >> 3;
  const unsigned cgb = (lane & 7) * 16;
  const unsigned rowb = (unsigned)(p.Wf + 2) * (4 * C) + cgb;      // sw cell of a footprint = nw + one bordered row
  const char* const fb = reinterpret_cast<const char*>(p.featT);
  f32x4 acc_s[kRDB], acc_q[kRDB];
#pragma unroll
  for (int k = 0; k < kRDB; ++k) acc_s[k] = acc_q[k] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int e = 0; e < ne; ++e) {
    psv_wave_sync<WPB>();                  // the previous pass is done with s_tap / s_P
    if (e % kMaxE == 0) {
      const int nload = min(kMaxE, ne - e) * 12;
#pragma unroll 1
      for (int i = lane; i < nload; i += 64) {
        const int src = p.edge_src[e_begin + e + i / 12];
        s_P[i / 12][i % 12] = p.camp[src * kCamStride + 24 + i % 12];
        if (i % 12 == 0) s_base[i / 12] = src * (p.Hf + 2) * (p.Wf + 2);      // cell (-1, -1) of the bordered map
      }
      psv_wave_sync<WPB>();
    }
    {
      float ix, iy;
      sample_position(s_P[e % kMaxE], X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
      s_tap[lane] = make_taps<4 * C>(ix, iy, p.Wf, p.Hf, s_base[e % kMaxE]);      // s_tap[pl1 * kRPix + px1]
    }
    psv_wave_sync<WPB>();
    unsigned c00 = ~0u;                // footprint held in t00..t11 (its nw cell pins all four)
    // deliberately not initialised: ~0 matches no offset, so the first plane always loads them
    f32x4 t00, t01, t10, t11;
#pragma unroll
    for (int pl = 0; pl < kRDB; ++pl) {
      const TapInfo ti = s_tap[pl * kRPix + gpx];
      if (ti.b00 != c00) {
        // (Reloading only the two new cells when the footprint moved by one cell -- register moves for the other two -- was
        // slower, 2.02 vs 1.84 ms: a step then issues two loads per direction the wave's pixels moved in, and the
        // vector-memory path is charged per wave instruction, not per active lane.)
        t00 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + cgb));
        t01 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + cgb) + 4 * C);
        t10 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + rowb));
        t11 = *reinterpret_cast<const f32x4*>(fb + (size_t)(ti.b00 + rowb) + 4 * C);
        c00 = ti.b00;
      }
      psv_blend_accumulate(t00, t01, t10, t11, ti, acc_s[pl], acc_q[pl]);
      // Finish this plane before the next one starts: the empty statement pins the accumulators here and, as a memory
      // barrier, keeps the next plane's tap-record read and footprint loads below it.  Without it the compiler issues the
      // (conditional) loads of all eight planes first, each into its own 16 registers: 136 VGPRs, 3 waves per SIMD, 21.9 ms.
      asm volatile("" : "+v"(acc_s[pl]), "+v"(acc_q[pl]) : : "memory");
    }
  }

  // ---- variance -> LDS -> stores ------------------------------------------------------------------------------
  psv_wave_sync<WPB>();
  const float cnt = (float)max(ne, 1);        // torch_scatter mean: sum / clamp(count, 1)
  // x / cnt is an IEEE division (~10 instructions); for a power-of-two count (8 views in the headline configuration)
  // x * (1 / cnt) is the same number exactly.  Wave-uniform choice.
  const bool cnt_pow2 = (max(ne, 1) & (max(ne, 1) - 1)) == 0;
  const float cnt_inv = 1.f / cnt;
  auto mean = [&](float x) __attribute__((always_inline)) { return cnt_pow2 ? x * cnt_inv : x / cnt; };
  const int cg = lane & 7;
  if constexpr (SPLIT) {
    // the lane's four channels are half `cg & 1` of channel group `cg / 2`; psv_split_slot trades halves with the partner lane:
    // the even lane stores the whole hi slot, the odd lane the whole lo slot; the 8 pixels of a wave make 128-byte runs
    const int chunk = cg >> 1, half = cg & 1;
    u32x4* const out = reinterpret_cast<u32x4*>(p.var);
    const int gp = ptile * kRPix + gpx;
#pragma unroll
    for (int pl = 0; pl < kRDB; ++pl) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = psv_variance_value(acc_s[pl][k], acc_q[pl][k], mean);
      const u32x4 slot = psv_split_slot(v, half);
      const int d = dchunk * kRDB + pl;
      if (gp < P && d < p.D) __builtin_nontemporal_store(slot, &out[(((size_t)r * 8 + chunk * 2 + half) * p.D + d) * P + gp]);
    }
  } else {
    // fp32 tensor: the four waves park kOutPl planes of their 8 pixels side by side ([plane][channel][32 pixels]) and the
    // workgroup stores every (channel, plane) row as one 128-byte run
    constexpr int NPX = WPB * kRPix;
    const int gp0 = (ptile - wv) * kRPix;             // first pixel of the workgroup
#pragma unroll
    for (int round = 0; round < kRDB / kOutPl; ++round) {
      if (round) __syncthreads();                      // the previous round's rows are stored
#pragma unroll
      for (int q = 0; q < kOutPl; ++q) {
        const int pl = round * kOutPl + q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          s_out[q][cg * 4 + k][wv * kRPix + gpx] = psv_variance_value(acc_s[pl][k], acc_q[pl][k], mean);
      }
      __syncthreads();
      for (int i = threadIdx.x; i < kOutPl * C * NPX; i += 64 * WPB) {
        const int q = i / (C * NPX), c = (i / NPX) % C, px = i % NPX;
        const int gp = gp0 + px, d = dchunk * kRDB + round * kOutPl + q;
        if (gp < P && d < p.D) __builtin_nontemporal_store(s_out[q][c][px], &p.var[(((size_t)r * C + c) * p.D + d) * P + gp]);
      }
    }
  }
}

}  // namespace

// Grid: (view, chunk of kGDB planes, tile of kGPix pixels), tiles fastest
int launch_psv_gather(PsvParams p, int C, int layout, hipStream_t s) {
  p.n_ptile = (p.h * p.w + kGPix - 1) / kGPix;
  const long long blocks = (long long)p.n_ref * ((p.D + kGDB - 1) / kGDB) * p.n_ptile;
  V3D_REQUIRE(blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: grid too large");
  const unsigned grid = (unsigned)blocks;
  if (layout == V3D_LAYOUT_SPLIT) psv_variance_kernel<32, true><<<grid, kGThreads, 0, s>>>(p);
  else if (C == 32) psv_variance_kernel<32, false><<<grid, kGThreads, 0, s>>>(p);
  else psv_variance_kernel<16, false><<<grid, kGThreads, 0, s>>>(p);
  V3D_CHECK_LAUNCH("psv_variance_kernel");
  return V3D_OK;
}

// Grid: (view, group of WPB 8-pixel tiles, chunk of kRDB planes), chunks fastest; four tiles per workgroup for the reference
// layout, one for the split layout
int launch_psv_reuse(PsvParams p, int layout, hipStream_t s) {
  const int n_tile = (p.h * p.w + kRPix - 1) / kRPix, n_dchunk = (p.D + kRDB - 1) / kRDB;
  V3D_REQUIRE((long long)p.n_ref * n_dchunk * n_tile < (1ll << 31), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: grid too large");
  const bool split = layout == V3D_LAYOUT_SPLIT;
  p.n_ptile = split ? n_tile : (n_tile + 3) / 4;
  const unsigned grid = (unsigned)((long long)p.n_ref * n_dchunk * p.n_ptile);
  if (split) psv_variance_reuse_kernel<true><<<grid, 64, 0, s>>>(p);
  else psv_variance_reuse_kernel<false><<<grid, 256, 0, s>>>(p);
  V3D_CHECK_LAUNCH("psv_variance_kernel");
  return V3D_OK;
}

}  // namespace v3d
