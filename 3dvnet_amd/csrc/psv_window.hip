// Plane-sweep warp + variance: the window kernel, its launch constants and its launcher (psv_variance.hip is the map of the
// family).  The kernel sits at the register limit of V3D_PSV_WAVES waves per SIMD: the empty asm statements in its body keep
// values out of vector registers, and an edit that looks neutral can spill (build.py checks that it does not).
#include "psv_kernels.h"

namespace v3d {
namespace {

// Window variant of the plane-reuse kernel (C == 32, 8 planes per wave), the default since round 3.
//
// Round-3 measurements behind it (scripts/micro/ta_mask.hip): a 16-byte-per-lane gather costs the CU's
// vector-memory path 7.2 ns per WAVE INSTRUCTION -- whatever the exec mask (8 or 64 active lanes) and whether a lane moves 8 or
// 16 bytes -- and the reuse kernel issues 1.8 of them per (plane, edge) step: 0.98 ms of its 1.65 ms per 64 cfg2 views are
// that path's busy time, queued behind each other (the ~1 300-cycle reload latency a wave sees).  Its reloads are mostly
// waste: a wave's 8 pixels x 8 planes x 1 edge touch 16 DISTINCT cells on average (the 2x2 footprints of neighbouring
// pixels and of consecutive planes overlap), the kernel loads 115 (forced reload of every pixel on the first plane, all four
// cells again when a footprint moves by one cell, masked lanes at full price).
//
// Here the wave takes the box spanned by the four corner samples of its 64 footprints per edge, cut to 16 x 4 cells (the whole
// box in 95 % of the passes at cfg2, 97 % at cfg5), and copies it into LDS with global_load_lds_dwordx4 -- one instruction
// per 8 cells of a row, no staging registers, 0.53 instructions per step instead of 1.8 -- and the footprints are read from
// there (ds_read_b128, a quarter of the L1 path's price per KB, tens instead of hundreds of cycles of latency).  Whether any
// pixel changes its footprint on plane k is known after the projection (one ballot): the reload branch is scalar and all
// lanes reload together.  A sample whose footprint lies outside the window (near planes with long epipolar slides, exotic
// camera pairs, the few tiles whose corners are not extreme) carries a flag in its tap word (the sign bit) and reads its four cells from
// featT as the reuse kernel does, inside the same step.  Arithmetic and accumulation order are those of the other two
// kernels: bit-identical output.
constexpr int kWinCols = 16, kWinRows = 4;                 // window: 16 x 4 cells x 128 B = 8 KB per wave
typedef float psv_f32x2 __attribute__((ext_vector_type(2)));

// scalar min / max of wave-uniform values (the compiler picks v_min3 / v_max3 + v_readfirstlane for these otherwise)
__device__ __forceinline__ int psv_smin(int a, int b) { int r; asm("s_min_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }
__device__ __forceinline__ int psv_smax(int a, int b) { int r; asm("s_max_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc"); return r; }

#ifndef V3D_PSVW_ABLATE
#define V3D_PSVW_ABLATE 0    // developer ablations of the window kernel: 1 no blend, 2 no footprint reads, 3 no window copy, 5 no store, 6 no out-of-window path
#endif
// CL8 (with SPLIT's geometry: one wave per workgroup, direct stores): the volume leaves as fp32 in the channel-last layout
// of the exact-fp32 depth-march conv0 (conv0z.hip) -- [n_ref][4 channel groups][2 halves][D][h][w] 16-byte slots of 4 floats
// (include/v3d.h, v3d_psv_variance_cl8): the split layout's addressing with the values themselves instead of bf16 pairs.
// WALK (depth walk, p.walk > 1): a wave keeps its 8 pixels for p.walk consecutive plane chunks.  WALK = false is the one-chunk
// kernel as it was before the walk: no chunk loop, and none of what the walk does to stay inside the registers of
// V3D_PSV_WAVES waves per SIMD (coordinates parked in LDS, values re-derived per chunk behind empty asm statements).
// Pass skip (p.skip, developer option "psv_skip"): a pass whose 64 samples all fall beside the source image adds exactly zero
// and keeps only the projection of the next edge (project() has the argument; 19 % of the passes at cfg2, 37 % at cfg5).
template <bool SPLIT, bool CL8 = false, bool WALK = false>
__global__ __launch_bounds__(SPLIT ? 64 : 256, V3D_PSV_WAVES) void psv_variance_window_kernel(PsvParams p) {
  static_assert(SPLIT || !CL8, "the channel-last fp32 output uses the single-wave geometry");
  constexpr int C = 32, WPB = SPLIT ? 1 : 4;
  constexpr unsigned CB = 4 * C;                            // bytes per cell
  constexpr int kOutPl = 4;                                 // planes staged per round of the fp32 epilogue
  static_assert(kWinCols == 16 && kRDB == 8 && kRPix == 8, "the window kernel projects one edge per pass: 8 planes x 8 pixels = 64 lanes");
  __shared__ __attribute__((aligned(16))) float s_win_[WPB][kWinRows * kWinCols * C];
  __shared__ __attribute__((aligned(16))) f32x4 s_w_[WPB][kRDB * kRPix];      // nw, ne, sw, se weights per (plane, pixel)
  __shared__ unsigned s_slot_[WPB][kRDB * kRPix];           // byte offset of the nw cell: in the window / in featT
  __shared__ float s_ref_[WPB][24];
  __shared__ float s_P_[WPB][kMaxE][12];
  __shared__ int s_base_[WPB][kMaxE];
  __shared__ __attribute__((aligned(16))) f32x4 s_xy_[WPB][WALK ? kRPix : 1];    // WALK: image coordinates (xf, yf) of the wave's 8 pixels
  // fp32 epilogue: [kOutPl][C][WPB * kRPix + 1] floats = 16.5 KB, parked on the four (by then dead) windows
  static_assert(SPLIT || kOutPl * C * (WPB * kRPix + 1) <= WPB * kWinRows * kWinCols * C, "epilogue staging fits the windows");

  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* const s_win = s_win_[wv];
  f32x4* const s_w = s_w_[wv];
  unsigned* const s_slot = s_slot_[wv];
  float* const s_ref = s_ref_[wv];
  float (*const s_P)[12] = s_P_[wv];
  int* const s_base = s_base_[wv];
  f32x4* const s_xy = s_xy_[wv];
  const unsigned b = (unsigned)v3d::xcd_contiguous_block();
  const unsigned b1 = v3d::udiv_magic(b, (unsigned)p.n_dseg, p.m_dseg), b2 = v3d::udiv_magic(b1, (unsigned)p.n_ptile, p.m_ptile);
  const int dseg = (int)(b - b1 * (unsigned)p.n_dseg);       // depth segments fastest (see the reuse kernel)
  // Depth walk: the wave keeps its 8 pixels for the chunks [c_begin, c_end) of its segment.  Between them only z differs: the
  // reference camera, the edges' camera blocks, the index arithmetic, the pixel coordinates and every launch constant below
  // are set up once per wave instead of once per chunk.
  const int c_begin = WALK ? dseg * p.walk : dseg, c_end = WALK ? min(c_begin + p.walk, p.n_dchunk) : c_begin + 1;
  const int ptile = (int)(b1 - b2 * (unsigned)p.n_ptile) * WPB + wv;
  const int r = (int)b2;
  const int P = p.h * p.w;
  const int e_begin = p.edge_ofs[r], e_end = p.edge_ofs[r + 1];
  const int ne = e_end - e_begin;
  const int ref = p.ref_img[r];
  if (lane < 21) s_ref[lane] = p.camp[ref * kCamStride + lane];

  // projection role: lane = (plane, pixel)
  const int pl1 = lane >> 3, px1 = lane & 7;
  const int gp1 = ptile * kRPix + px1;
  float xf1, yf1;                          // (WALK = false: the coordinates stay in registers)
  {
    // row / column of the lane's pixel: the wave's first pixel is divided once (wave-uniform), the lane adds its offset
    // (rows of at least kRPix pixels wrap at most once)
    int gy, gx;
    if (p.w >= kRPix) {
      const unsigned g0 = (unsigned)(ptile * kRPix), gy0 = v3d::udiv_magic(g0, (unsigned)p.w, p.m_w);
      gx = (int)(g0 - gy0 * (unsigned)p.w) + px1;
      gy = (int)gy0;
      if (gx >= p.w) { gx -= p.w; ++gy; }
    } else {
      gy = gp1 / p.w; gx = gp1 % p.w;
    }
    const float xf = (p.w > 1 && gx == p.w - 1) ? (float)(p.W - 1) : (float)((double)gx * p.x_step);
    const float yf = (p.h > 1 && gy == p.h - 1) ? (float)(p.H - 1) : (float)((double)gy * p.y_step);
    // parked in LDS for the walk (the lanes of plane 0 write; every chunk reads them back: one ds_read_b64 instead of two
    // registers held across the whole kernel, which sits at the register limit of V3D_PSV_WAVES waves per SIMD)
    if constexpr (WALK) { if (pl1 == 0) s_xy[px1] = (f32x4){xf, yf, 0.f, 0.f}; }
    xf1 = xf; yf1 = yf;
  }
  psv_wave_sync<WPB>();
  // per chunk (set at the top of the chunk loop): the lane's world point, and whether its (pixel, plane) exists
  float X, Y, Z;
  bool live1, all_live;
  unsigned long long live_mask;           // ballot of live1 (wave-uniform)
  const float Wm1 = (float)(p.W - 1), Hm1 = (float)(p.H - 1);
  const float rWm1 = p.rWm1, rHm1 = p.rHm1;
  const float Wfm1 = (float)(p.Wf - 1), Hfm1 = (float)(p.Hf - 1);
  const int Wp = p.Wf + 2;
  const float Wff = (float)p.Wf, Hff = (float)p.Hf;
  const bool skip_on = p.skip != 0;

  // gather role: 8 lanes x float4 per pixel
  const int gpx = lane >> 3;
  const unsigned cgb = (lane & 7) * 16;
  const unsigned rowb = (unsigned)Wp * CB + cgb;
  const unsigned lane16 = (unsigned)lane * 16u;
  const char* const fb = reinterpret_cast<const char*>(p.featT);
  const char* const wb = reinterpret_cast<const char*>(s_win);
  // LDS byte address of this wave's window (what M0 carries for global_load_lds)
  const unsigned win_lds = __builtin_amdgcn_readfirstlane(
      (unsigned)(size_t)(__attribute__((address_space(3))) void*)s_win);
  f32x4 acc_s[kRDB], acc_q[kRDB];

#if V3D_PSVW_ABLATE == 1
#define V3D_PSV_BLEND(pl_, w_) asm volatile("" : : "v"(t00), "v"(t01), "v"(t10), "v"(t11), "v"(w_) : "memory")
#else
#define V3D_PSV_BLEND(pl_, w_)                                                                       \
  do {                                                                                               \
    f32x4 sv_ = t00 * (w_)[0];                                                                       \
    sv_ = __builtin_elementwise_fma(t01, (f32x4){(w_)[1], (w_)[1], (w_)[1], (w_)[1]}, sv_);          \
    sv_ = __builtin_elementwise_fma(t10, (f32x4){(w_)[2], (w_)[2], (w_)[2], (w_)[2]}, sv_);          \
    /* fourth tap: hipcc copies w[3] into the low half of a register pair first (one v_mov per plane); written by hand  \
       the packed FMA takes the HIGH half of the (w[2], w[3]) pair for both result lanes (op_sel) -- same arithmetic */ \
    {                                                                                                \
      psv_f32x2 lo_ = {sv_[0], sv_[1]}, hi_ = {sv_[2], sv_[3]};                                      \
      const psv_f32x2 w23_ = {(w_)[2], (w_)[3]};                                                     \
      const psv_f32x2 tl_ = {t11[0], t11[1]}, th_ = {t11[2], t11[3]};                                \
      asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(lo_) : "v"(tl_), "v"(w23_));  \
      asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(hi_) : "v"(th_), "v"(w23_));  \
      sv_ = (f32x4){lo_[0], lo_[1], hi_[0], hi_[1]};                                                 \
    }                                                                                                \
    acc_s[pl_] += sv_;                                                                               \
    acc_q[pl_] = __builtin_elementwise_fma(sv_, sv_, acc_q[pl_]);                                    \
    /* finish this plane before the next one starts (see the reuse kernel) */                        \
    asm volatile("" : "+v"(acc_s[pl_]), "+v"(acc_q[pl_]) : : "memory");                              \
  } while (0)
#endif

  // camera blocks (P = K [R|t], first cell of the bordered map) of edges e0 .. e0 + 7
  auto load_cams = [&](int e0) __attribute__((always_inline)) {
    const int nload = min(kMaxE, ne - e0) * 12;
    // (the lane index goes through an empty statement: the compiler otherwise works out the lane's addresses before the walk and
    // holds them in vector registers across the whole kernel)
    int lane0 = lane;
    if constexpr (WALK) asm volatile("" : "+v"(lane0));
#pragma unroll 1
    for (int i = lane0; i < nload; i += 64) {
      const int src = p.edge_src[e_begin + e0 + i / 12];
      s_P[i / 12][i % 12] = p.camp[src * kCamStride + 24 + i % 12];
      if (i % 12 == 0) s_base[i / 12] = src * (p.Hf + 2) * Wp;      // cell (-1, -1) of the bordered map
    }
  };
  // projection of this lane's (pixel, plane) sample into the source view of edge e (make_taps, spelled out: the cell
  // coordinates are needed): nw cell of the footprint in the bordered map (x0 + 1, y0 + 1) + the four bilinear weights
  auto project = [&](int e, int& xb, int& yb, f32x4& wq, bool& skip) __attribute__((always_inline)) {
    float ix, iy;
    v3d::sample_position(s_P[e % kMaxE], X, Y, Z, Wm1, rWm1, Hm1, rHm1, Wfm1, Hfm1, ix, iy);
    // clamp to [-1, Wf] x [-1, Hf] (make_taps): v_med3_f32 returns the smallest number when an operand is NaN, i.e. -1,
    // what fminf(fmaxf(NaN, -1), Wf) gives
    ix = __builtin_amdgcn_fmed3f(ix, -1.f, Wff);
    iy = __builtin_amdgcn_fmed3f(iy, -1.f, Hff);
    // Pass skip.  A sample clamped onto -1 or Wf (Hf) lies wholly beside the source image (NaN coordinates clamp to -1): every
    // cell of its footprint is a border cell (+0) or carries the weight 0, so for finite features its blend sv_ is +-0 (weights
    // are >= 0).  An accumulator starts at +0 and can never become -0 under round-to-nearest (x + y is -0 only for x = y = -0),
    // hence acc + (+-0) and fma(+-0, +-0, acc) leave every accumulator bit as it is: a pass whose 64 samples are all such
    // samples (lanes without a sample count as one) changes nothing and is left out.  The test is exact -- a sample at
    // -1 < ix < 0 has a weight on column 0 and is not zero -- and wave-uniform: the flag lives in scalar registers.
    // (four ballots joined in scalar registers: one v_cmp each; __all() of the joined condition goes through a 0 / 1 vector
    // register and a fifth compare)
    skip = skip_on && (__ballot(ix != -1.f) & __ballot(ix != Wff) & __ballot(iy != -1.f) & __ballot(iy != Hff) & live_mask) == 0;
    const float x0 = floorf(ix), y0 = floorf(iy);
    const float x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float wx0 = x1 - ix, wx1 = ix - x0, wy0 = y1 - iy, wy1 = iy - y0;
    wq = (f32x4){v3d::mul_rn(wx0, wy0), v3d::mul_rn(wx1, wy0), v3d::mul_rn(wx0, wy1), v3d::mul_rn(wx1, wy1)};
    xb = (int)x0 + 1;
    yb = (int)y0 + 1;
    // lanes beyond the plane grid / the last plane must not stretch the box: they take lane 0's cell (always live) -- read
    // under full exec (inside a branch on !live1 readfirstlane would return the first DEAD lane's own value)
    // (wave-uniform skip: only the waves on the last pixels of the plane grid / the last planes have such lanes)
    if (!all_live) {
      const int xb0 = __builtin_amdgcn_readlane(xb, 0), yb0 = __builtin_amdgcn_readlane(yb, 0);
      xb = live1 ? xb : xb0;
      yb = live1 ? yb : yb0;
    }
  };
  // Software pipeline over the edges: the samples of edge e + 1 are projected while the window of edge e is on its way
  // from L2 to LDS (the copy's latency was 0.27 of 1.59 ms when the wave simply waited for it)
  int xb = 0, yb = 0;
  f32x4 wq = {0.f, 0.f, 0.f, 0.f};
  bool skip = false;                       // wave-uniform: the pass that (xb, yb, wq) belong to adds exactly zero
  if (ne > 0) {
    load_cams(0);
    psv_wave_sync<WPB>();
  }
  const bool cnt_pow2 = (max(ne, 1) & (max(ne, 1) - 1)) == 0;
  const int cg = lane & 7;

  for (int dchunk = c_begin; dchunk < c_end; ++dchunk) {
    const int d1 = dchunk * kRDB + pl1;
    {
      // (the empty statement keeps the plane range in scalar registers: hoisted out of the walk, its vector-register copies
      // are live across the whole kernel and spill)
      double z_start = p.z_start, z_end = p.z_end;
      if constexpr (WALK) asm volatile("" : "+s"(z_start), "+s"(z_end));
      const float z = (d1 == p.D - 1 && p.D > 1) ? (float)z_end : (float)(z_start + (double)d1 * p.z_step);
      if constexpr (WALK) {
        const f32x4 xy = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(s_xy) + cgb);      // s_xy[px1]
        xf1 = xy[0]; yf1 = xy[1];
      }
      v3d::world_point(s_ref, xf1, yf1, z, X, Y, Z);
    }
    live1 = gp1 < P && d1 < p.D;                              // lane 0 is always live
    live_mask = __ballot(live1);
    all_live = __all(live1);
#pragma unroll
    for (int k = 0; k < kRDB; ++k) acc_s[k] = acc_q[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ne > 0) {
      // more edges than s_P holds: the previous chunk's last pass left edges 8.. there
      if (ne > kMaxE && dchunk != c_begin) {
        psv_wave_sync<WPB>();
        load_cams(0);
        psv_wave_sync<WPB>();
      }
      project(0, xb, yb, wq, skip);
    }
    for (int e = 0; e < ne; ++e) {
      psv_wave_sync<WPB>();                  // the previous pass is done with s_w / s_slot / s_win
#ifdef V3D_PSV_NOPIPE                      // developer A/B: project at the top of the pass, wait for the copy right after issuing it
      if (e > 0) {
        if (e % kMaxE == 0) { load_cams(e); psv_wave_sync<WPB>(); }
        project(e, xb, yb, wq, skip);
      }
#endif
      // A skipped pass (see project()) keeps only the projection of the next edge and the camera reloads: no box, no tap
      // records, no window copy, no wait, no plane loop.  The mean still divides by ne: the edge counts, its samples are zeros.
      unsigned long long chg = 0;
      if (!skip) {
        // Window = the box spanned by the four corner samples (first / last pixel on the first / last plane: a projective map is
        // monotone in pixel and in depth, so they bound the 64 footprints in all but a few tiles), cut to 16 x 4 cells.  A
        // sample whose footprint is not inside it is simply marked (bit 0 of its tap word) and takes its cells from featT.
        int xmin, ymin, ncol, nrow;            // wave-uniform
        {
          // (both coordinates of a corner travel in one word: four lane reads instead of eight; bordered coordinates are >= 0)
          const int cc = (yb << 16) | xb;
          const int ca = __builtin_amdgcn_readlane(cc, 0), cb = __builtin_amdgcn_readlane(cc, 7);
          const int cd = __builtin_amdgcn_readlane(cc, 56), ce = __builtin_amdgcn_readlane(cc, 63);
          const int xa = ca & 0xffff, xc = cb & 0xffff, xd = cd & 0xffff, xe = ce & 0xffff;
          const int ya = ca >> 16, yc = cb >> 16, yd = cd >> 16, ye = ce >> 16;
          xmin = psv_smin(psv_smin(xa, xc), psv_smin(xd, xe));
          ymin = psv_smin(psv_smin(ya, yc), psv_smin(yd, ye));
          ncol = psv_smax(psv_smax(xa, xc), psv_smax(xd, xe)) - xmin + 2 > 8 ? kWinCols : 8;
          nrow = psv_smin(psv_smax(psv_smax(ya, yc), psv_smax(yd, ye)) - ymin + 2, kWinRows);
        }
        const int base_cell = __builtin_amdgcn_readfirstlane(s_base[e % kMaxE]);
        const unsigned dx = (unsigned)(xb - xmin), dy = (unsigned)(yb - ymin);
        const bool inwin = dx <= (unsigned)(ncol - 2) && dy <= (unsigned)(nrow - 2);
        // tap word: byte offset of the nw cell in the window, or -- sign bit set -- in featT (< 2 GB, checked by the host)
        const unsigned so_win = ((dy << 4) | dx) * CB;
        const unsigned so_ext = ((unsigned)(base_cell + __mul24(yb, Wp) + xb) * CB) | 0x80000000u;
        const unsigned so = inwin ? so_win : so_ext;
        s_w[lane] = wq;
        s_slot[lane] = so;
        // does ANY pixel change its footprint on plane k (bit group k of the ballot)?  plane 0 always loads
        const unsigned prev = (unsigned)__builtin_amdgcn_ds_bpermute(((lane - 8) & 63) * 4, (int)so);
        chg = __ballot(lane < 8 || so != prev);
        // copy the window: nrow rows of 8 or 16 cells from (xmin, ymin) (runs past the last needed column stay inside the bordered
        // maps + tail); lane l moves bytes [16 l, 16 l + 16) of each 1 KB run
        {
          // wave-uniform row address (SGPR pair) + the lane's 16 bytes (one constant VGPR): no per-lane address arithmetic.  The
          // copies are written in assembly (hipcc forms 64-bit per-lane addresses for the builtin): M0 = LDS byte address of the
          // run, saved and restored around each copy; the wave waits for them itself (vmcnt below).
          const char* rowp = fb + (size_t)((unsigned)(base_cell + ymin * Wp + xmin) * CB);
          unsigned dst = win_lds;
          asm volatile("s_nop 4" ::: "memory");            // SGPRs written by v_readlane may feed the first copy's address
#pragma unroll 1
          for (int rr = 0; rr < (V3D_PSVW_ABLATE == 3 ? 0 : nrow); ++rr) {
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(lane16), "s"(rowp), "s"(dst) : "memory");
            if (ncol > 8)
              asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024\n\ts_mov_b32 m0, %0"
                           : "=&s"(keep) : "v"(lane16), "s"(rowp), "s"(dst) : "memory");   // the instruction offset moves BOTH addresses
            rowp += (size_t)Wp * CB;
            dst += kWinCols * CB;
          }
        }
      }      // !skip
      bool skip_next = false;
#ifndef V3D_PSV_NOPIPE
      if (e + 1 < ne) {
        if ((e + 1) % kMaxE == 0) {
          psv_wave_sync<WPB>();
          load_cams(e + 1);
          psv_wave_sync<WPB>();
        }
        project(e + 1, xb, yb, wq, skip_next);
      }
#endif
      if (!skip) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // the window has landed, the tap records are written
        psv_wave_sync<WPB>();
        // deliberately not initialised: the first plane of a pass always loads them
        f32x4 t00, t01, t10, t11;
        f32x4 wn = s_w[gpx];
        unsigned sn = s_slot[gpx];
#pragma unroll
        for (int pl = 0; pl < kRDB; ++pl) {
          const f32x4 w = wn;
          const unsigned so_pl = sn;
          if (pl + 1 < kRDB) {               // next plane's record: in flight during this plane's blend
            wn = s_w[(pl + 1) * kRPix + gpx];
            sn = s_slot[(pl + 1) * kRPix + gpx];
          }
          if (((chg >> (8 * pl)) & 0xffull) && (V3D_PSVW_ABLATE != 2 || (pl == 0 && e == 0))) {      // wave-uniform: all pixels reload together (a load costs the same masked or not)
            // (a wave-uniform test "no sample of this plane is outside the window" -- one ballot per pass -- in front of the per-lane
            // sign test saves a v_cmp and the exec-mask juggling in 95 % of the planes and measured 0.6 % SLOWER, round 4)
            if (V3D_PSVW_ABLATE != 6 && (int)so_pl < 0) {
              const unsigned b00 = so_pl & 0x7fffffffu;
              t00 = *reinterpret_cast<const f32x4*>(fb + (size_t)(b00 + cgb));
              t01 = *reinterpret_cast<const f32x4*>(fb + (size_t)(b00 + cgb) + CB);
              t10 = *reinterpret_cast<const f32x4*>(fb + (size_t)(b00 + rowb));
              t11 = *reinterpret_cast<const f32x4*>(fb + (size_t)(b00 + rowb) + CB);
            } else {
              const char* a = wb + (so_pl + cgb);
              t00 = *reinterpret_cast<const f32x4*>(a);
              t01 = *reinterpret_cast<const f32x4*>(a + CB);
              t10 = *reinterpret_cast<const f32x4*>(a + kWinCols * CB);
              t11 = *reinterpret_cast<const f32x4*>(a + kWinCols * CB + CB);
            }
          }
          V3D_PSV_BLEND(pl, w);
        }
      }      // !skip
      skip = skip_next;
    }

    // ---- variance -> stores (as in the reuse kernel) -------------------------------------------------------------
    psv_wave_sync<WPB>();
    // (the thread index of the store addresses goes through an empty statement, as in load_cams: worked out before the walk, the
    // lanes' 64-bit addresses would be held in vector registers across the whole kernel)
    int tid_o = (int)threadIdx.x;
    if constexpr (WALK) asm volatile("" : "+v"(tid_o));
    int ne_o = ne;                                // (likewise the mean's divisor and its reciprocal: a dozen instructions per chunk)
    if constexpr (WALK) asm volatile("" : "+s"(ne_o));
    const float cnt = (float)max(ne_o, 1);        // torch_scatter mean: sum / clamp(count, 1)
    const float cnt_inv = 1.f / cnt;
    if constexpr (SPLIT) {
      const int chunk = cg >> 1, half = cg & 1;
      u32x4* const out = reinterpret_cast<u32x4*>(p.var);
      const int gp = ptile * kRPix + (tid_o >> 3);
      // the lane's slot on the chunk's first plane; plane pl is pl * P slots further (a wave-uniform stride: with the whole
      // index spelled out per plane the compiler rebuilt the 64-bit product -- two v_mul_lo_u32 and a v_mad_u64_u32 -- eight times).
      // WALK: wave-uniform 64-bit part + the lane's 32-bit slot inside its view's volume (8 D P slots < 2^32, checked by the
      // host): nothing of it is held in vector registers across the walk.
      u32x4* const obase = WALK ? out + ((size_t)r * 8 * p.D + (size_t)dchunk * kRDB) * P +
                                      ((unsigned)(chunk * 2 + half) * (unsigned)(p.D * P) + (unsigned)gp)
                                : out + (((size_t)r * 8 + chunk * 2 + half) * p.D + (size_t)dchunk * kRDB) * P + gp;
      // x / cnt is an IEEE division; for a power-of-two count x * (1 / cnt) is the same number exactly.  ONE wave-uniform
      // branch around the whole epilogue (the reuse kernel tests it per value: 64 branches)
#define V3D_PSV_EMIT(MEAN)                                                                                              \
    _Pragma("unroll") for (int pl = 0; pl < kRDB; ++pl) {                                                               \
      float v[4];                                                                                                       \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                   \
        const float avg = MEAN(acc_s[pl][k]);                                                                           \
        const float avg_sq = MEAN(acc_q[pl][k]);                                                                        \
        v[k] = v3d::sub_rn(avg_sq, v3d::mul_rn(avg, avg));                    /* mvsnet.py:216 */                       \
      }                                                                                                                 \
      const int d = dchunk * kRDB + pl;                                                                                 \
      if constexpr (CL8) {                                                                                              \
        /* channels 4 cg .. 4 cg + 3 = half `half` of the voxel's channel group `chunk`: the lane's own 16 bytes */       \
        const u32x4 slot = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};\
        if (gp < P && d < p.D)                                                                                          \
          __builtin_nontemporal_store(slot, obase + (size_t)pl * (unsigned)P);                                           \
      } else {                                                                                                          \
      const unsigned h01 = pack_bf16x2(v[0], v[1]), h23 = pack_bf16x2(v[2], v[3]);                                      \
      const unsigned l01 = pack_bf16x2(v[0] - __uint_as_float(h01 << 16), v[1] - __uint_as_float(h01 & 0xffff0000u));   \
      const unsigned l23 = pack_bf16x2(v[2] - __uint_as_float(h23 << 16), v[3] - __uint_as_float(h23 & 0xffff0000u));   \
      const unsigned s0 = half ? h01 : l01, s1 = half ? h23 : l23;             /* what the partner lane stores */        \
      const unsigned r0 = (unsigned)__builtin_amdgcn_mov_dpp((int)s0, 0xB1, 0xf, 0xf, true);   /* quad_perm [1,0,3,2] */ \
      const unsigned r1 = (unsigned)__builtin_amdgcn_mov_dpp((int)s1, 0xB1, 0xf, 0xf, true);                            \
      const u32x4 slot = half ? (u32x4){r0, r1, l01, l23} : (u32x4){h01, h23, r0, r1};                                  \
      if (gp < P && d < p.D && (V3D_PSVW_ABLATE != 5 || slot[0] == 0x12345u))                                           \
        __builtin_nontemporal_store(slot, obase + (size_t)pl * (unsigned)P);                                             \
      }                                                                                                                 \
    }
#define V3D_MEAN_MUL(x) ((x) * cnt_inv)
      // any other count: the correctly rounded quotient from the correctly rounded reciprocal (v3d::div_uniform, Markstein;
      // 4 instructions instead of the 11 of the IEEE sequence, twice per output value); v_div_fixup restores the special cases
#define V3D_MEAN_DIV(x) __builtin_amdgcn_div_fixupf(v3d::div_uniform((x), cnt, cnt_inv), cnt, (x))
      if (cnt_pow2) { V3D_PSV_EMIT(V3D_MEAN_MUL) } else { V3D_PSV_EMIT(V3D_MEAN_DIV) }
#undef V3D_PSV_EMIT
#undef V3D_MEAN_MUL
#undef V3D_MEAN_DIV
    } else {
      constexpr int NPX = WPB * kRPix;
      float (*const s_out)[C][NPX + 1] = reinterpret_cast<float (*)[C][NPX + 1]>(&s_win_[0][0]);
      auto mean = [&](float x) __attribute__((always_inline)) {
        return cnt_pow2 ? x * cnt_inv : __builtin_amdgcn_div_fixupf(v3d::div_uniform(x, cnt, cnt_inv), cnt, x);
      };
      const int gp0 = (ptile - wv) * kRPix;             // first pixel of the workgroup
#pragma unroll
      for (int round = 0; round < kRDB / kOutPl; ++round) {
        __syncthreads();                                 // every wave is done with its window / the previous round is stored
#pragma unroll
        for (int q = 0; q < kOutPl; ++q) {
          const int pl = round * kOutPl + q;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float avg = mean(acc_s[pl][k]);
            const float avg_sq = mean(acc_q[pl][k]);
            s_out[q][cg * 4 + k][wv * kRPix + gpx] = v3d::sub_rn(avg_sq, v3d::mul_rn(avg, avg));   // mvsnet.py:216
          }
        }
        __syncthreads();
        for (int i = tid_o; i < kOutPl * C * NPX; i += 64 * WPB) {
          const int q = i / (C * NPX), c = (i / NPX) % C, px = i % NPX;
          const int gp = gp0 + px, d = dchunk * kRDB + round * kOutPl + q;
          if (gp < P && d < p.D) __builtin_nontemporal_store(s_out[q][c][px], &p.var[(((size_t)r * C + c) * p.D + d) * P + gp]);
        }
      }
      // the staged rows live on the windows: all four waves (they walk the same segment) have read them before the next chunk's
      // window copies land there
      if (WALK && dchunk + 1 < c_end) __syncthreads();
    }
  }      // chunk loop
#undef V3D_PSV_BLEND
}

// Plane chunks a wave walks (PsvParams::walk).  A longer walk spreads the per-wave set-up over more chunks but leaves fewer,
// longer waves, i.e. a longer tail behind the last full round of resident waves.  The rule is a function of the shape alone --
// the same for every call of a shape: the longest walk that keeps the launch at kMinRounds rounds of the kResident waves an
// MI355X holds (256 CUs x 4 SIMDs x V3D_PSV_WAVES), evened out over the segments (5 chunks at a walk of 4 are 3 + 2, not
// 4 + 1).  `forced` > 0 (developer option "psv_walk") overrides it.
int psv_walk_chunks(int forced, int n_dchunk, int n_ref, int n_ptile) {
  constexpr long long kResident = 256 * 4 * V3D_PSV_WAVES, kMinRounds = 16;
  long long walk = forced > 0 ? forced : (long long)n_ref * n_dchunk * n_ptile / (kMinRounds * kResident);
  walk = walk < 1 ? 1 : walk > n_dchunk ? n_dchunk : walk;
  if (forced > 0) return (int)walk;
  const long long n_dseg = (n_dchunk + walk - 1) / walk;
  return (int)((n_dchunk + n_dseg - 1) / n_dseg);
}

}  // namespace

// Grid: (view, group of WPB 8-pixel tiles, depth segment), segments fastest.  The reference layout takes four tiles per
// workgroup (128-byte rows of the fp32 tensor), the split and cl8 layouts one.
int launch_psv_window(PsvParams p, int layout, hipStream_t s) {
  const bool single = layout != V3D_LAYOUT_REFERENCE;
  const int n_tile = (p.h * p.w + kRPix - 1) / kRPix;
  p.n_dchunk = (p.D + kRDB - 1) / kRDB;
  V3D_REQUIRE((long long)p.n_ref * p.n_dchunk * n_tile < (1ll << 31), V3D_ERR_BAD_SHAPE, "v3d_psv_variance_f32: grid too large");
  p.n_ptile = single ? n_tile : (n_tile + 3) / 4;
  p.walk = psv_walk_chunks(option(kOptPsvWalk), p.n_dchunk, p.n_ref, n_tile);
  // the walking kernel addresses a lane's split / cl8 output slot inside its view's volume with 32 bits
  if (single && 8ull * p.D * p.h * p.w >= (1ull << 32)) p.walk = 1;
  p.n_dseg = (p.n_dchunk + p.walk - 1) / p.walk;
  p.skip = option(kOptPsvSkip) != 0;
  const unsigned long long nblk = (unsigned long long)p.n_ref * p.n_dseg * p.n_ptile;
  p.rWm1 = (float)(1.0 / (double)(p.W - 1));
  p.rHm1 = (float)(1.0 / (double)(p.H - 1));
  p.m_dseg = magic_u32(nblk, (unsigned)p.n_dseg);
  p.m_ptile = magic_u32(nblk / p.n_dseg + 1, (unsigned)p.n_ptile);
  p.m_w = magic_u32((unsigned long long)p.h * p.w + 4 * kRPix, (unsigned)p.w);
  const unsigned grid = (unsigned)nblk;
  const bool walk = p.walk > 1;      // one chunk per wave: the kernel without the walk's bookkeeping
  if (layout == V3D_LAYOUT_CL8) {
    if (walk) psv_variance_window_kernel<true, true, true><<<grid, 64, 0, s>>>(p);
    else psv_variance_window_kernel<true, true, false><<<grid, 64, 0, s>>>(p);
  } else if (layout == V3D_LAYOUT_SPLIT) {
    if (walk) psv_variance_window_kernel<true, false, true><<<grid, 64, 0, s>>>(p);
    else psv_variance_window_kernel<true, false, false><<<grid, 64, 0, s>>>(p);
  } else {
    if (walk) psv_variance_window_kernel<false, false, true><<<grid, 256, 0, s>>>(p);
    else psv_variance_window_kernel<false, false, false><<<grid, 256, 0, s>>>(p);
  }
  V3D_CHECK_LAUNCH("psv_variance_kernel");
  return V3D_OK;
}

}  // namespace v3d

extern "C" int v3d_psv_walk_chunks(int n_ref, int D, int h, int w) {
  using namespace v3d;
  V3D_REQUIRE(n_ref > 0 && D > 0 && h > 0 && w > 0, V3D_ERR_BAD_SHAPE, "v3d_psv_walk_chunks: bad shape");
  return psv_walk_chunks(option(kOptPsvWalk), (D + kRDB - 1) / kRDB, n_ref, (h * w + kRPix - 1) / kRPix);
}

