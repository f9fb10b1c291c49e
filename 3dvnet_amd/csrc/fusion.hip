// Multi-view depth fusion (mv3d/eval/pointcloudfusion_custom.py: process_depth / process_scene): the depth maps of a scene ->
// one fused, colour-carrying point cloud.  Every pixel of a reference view is lifted to the world, projected into each source
// view, compared with that view's depth at the nearest texel, and the consistent samples are averaged.
//
//   fuse_depths_kernel     one thread per reference pixel walks the source list in order; the whole per-pair chain (project,
//                          two divisions, normalise / un-normalise, round, one 4-byte gather, back-project) stays in registers.
//                          Dense outputs pts [n_ref, h w, 3] and n_valid [n_ref, h w], written once.  No atomics, no LDS, no
//                          scratch (build-time ISA guard): the per-thread sum runs in ascending list order, so repeated launches
//                          are bit-identical.
//   fusion_compact_*       keep mask, per-tile counts, one-workgroup exclusive scan, ordered scatter of the kept points and colours
//                          in (view, pixel) order; the total lands in a device word.
//
// Arithmetic: the rounding points are those of the reference's fp32 tensor program: 3x3 . 3-vector products as
// k-ordered chains whose first term is a plain product, translations as separate rounded additions, IEEE divisions for u, v
// and the final average, grid_sample's normalise / un-normalise round trip spelled out, round-half-even for the texel.  The
// reference's NaN-zeroing branch (pointcloudfusion_custom.py:85-87) needs no counterpart: a sample can only be NaN when z = 0
// or the texel lies outside the image, and such a source fails z > 1e-4 / the bounds test, so it is never summed here.
#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::dot3_chain;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kCam = 48;      // floats per camera block: [0..8] K, [9..17] K^-1, [18..26] R, [27..29] t, [30..41] top 3 rows of P^-1
constexpr int kTile = 256;    // pixels (= threads) per workgroup

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// `edge_ofs` == nullptr: the sources of reference r are all other images in ascending order.
__global__ __launch_bounds__(kTile) void fuse_depths_kernel(const float* __restrict__ depths, const float* __restrict__ cams,
                                                             const int* __restrict__ ref_img, const int* __restrict__ edge_ofs,
                                                             const int* __restrict__ edge_src, int n_img, int hw, int w, int h,
                                                             int tiles_per_view, unsigned tiles_magic, float z_thresh,
                                                             float* __restrict__ pts, int* __restrict__ n_valid) {
  // consecutive workgroups of an XCD sit on neighbouring tiles of the same reference view
  const int blk = v3d::xcd_contiguous_block();
  const int r = (int)v3d::udiv_magic((unsigned)blk, (unsigned)tiles_per_view, tiles_magic);
  const int p = (blk - r * tiles_per_view) * kTile + (int)threadIdx.x;
  if (p >= hw) return;
  const int ri = ref_img ? ref_img[r] : r;
  if ((unsigned)ri >= (unsigned)n_img) return;                 // validated on the host; never index outside the stack
  const float* __restrict__ cr = cams + (size_t)ri * kCam;     // wave-uniform address: scalar loads

  const int y = p / w, x = p - y * w;
  const float d = depths[(size_t)ri * hw + p];
  const float Wm1 = (float)(w - 1), Hm1 = (float)(h - 1);
  const float rWm1 = div_rn(1.f, Wm1), rHm1 = div_rn(1.f, Hm1);

  // X = P^-1[:3,:3] (K^-1 [x d, y d, d]) + P^-1[:3,3]
  float X, Y, Z;
  {
    const float p0 = mul_rn((float)x, d), p1 = mul_rn((float)y, d), p2 = d;
    const float c0 = dot3_chain(cr[9], p0, cr[10], p1, cr[11], p2);
    const float c1 = dot3_chain(cr[12], p0, cr[13], p1, cr[14], p2);
    const float c2 = dot3_chain(cr[15], p0, cr[16], p1, cr[17], p2);
    X = add_rn(dot3_chain(cr[30], c0, cr[31], c1, cr[32], c2), cr[33]);
    Y = add_rn(dot3_chain(cr[34], c0, cr[35], c1, cr[36], c2), cr[37]);
    Z = add_rn(dot3_chain(cr[38], c0, cr[39], c1, cr[40], c2), cr[41]);
  }

  float sx = X, sy = Y, sz = Z;
  int nv = 0;
  const int j0 = edge_ofs ? edge_ofs[r] : 0;
  const int j1 = edge_ofs ? edge_ofs[r + 1] : n_img;
  for (int j = j0; j < j1; ++j) {
    const int s = edge_ofs ? edge_src[j] : j;
    if ((!edge_ofs && s == ri) || (unsigned)s >= (unsigned)n_img) continue;      // uniform branch
    const float* __restrict__ cs = cams + (size_t)s * kCam;
    // q = K (R X + t)
    const float a0 = add_rn(dot3_chain(cs[18], X, cs[19], Y, cs[20], Z), cs[27]);
    const float a1 = add_rn(dot3_chain(cs[21], X, cs[22], Y, cs[23], Z), cs[28]);
    const float a2 = add_rn(dot3_chain(cs[24], X, cs[25], Y, cs[26], Z), cs[29]);
    const float qx = dot3_chain(cs[0], a0, cs[1], a1, cs[2], a2);
    const float qy = dot3_chain(cs[3], a0, cs[4], a1, cs[5], a2);
    const float z = dot3_chain(cs[6], a0, cs[7], a1, cs[8], a2);
    const float u = div_rn(qx, z), v = div_rn(qy, z);
    // a NaN coordinate (z = 0) fails every comparison
    const bool inside = z > 1e-4f && u >= 0.f && u <= Wm1 && v >= 0.f && v <= Hm1;
    if (!inside) continue;
    // grid_sample(nearest, align_corners=True): g = (u / (w-1)) * 2 - 1 (the doubling is exact: one rounding, at the
    // subtraction), i = ((g + 1) / 2) * (w-1) (the halving is exact), texel = round-half-even(i); zero outside the image
    const float gx = sub_rn(mul_rn(v3d::div_uniform(u, Wm1, rWm1), 2.f), 1.f);
    const float gy = sub_rn(mul_rn(v3d::div_uniform(v, Hm1, rHm1), 2.f), 1.f);
    const float fx = __builtin_rintf(mul_rn(mul_rn(add_rn(gx, 1.f), 0.5f), Wm1));
    const float fy = __builtin_rintf(mul_rn(mul_rn(add_rn(gy, 1.f), 0.5f), Hm1));
    float zs = 0.f;
    if (fx >= 0.f && fx <= Wm1 && fy >= 0.f && fy <= Hm1) zs = depths[(size_t)s * hw + (int)fy * w + (int)fx];
    if (!(fabsf(sub_rn(z, zs)) < z_thresh)) continue;
    // X_s = R^T (K^-1 [u z_s, v z_s, z_s] - t)   (the third homogeneous coordinate z / z is exactly 1 for z > 1e-4)
    const float b0 = mul_rn(u, zs), b1 = mul_rn(v, zs);
    const float e0 = sub_rn(dot3_chain(cs[9], b0, cs[10], b1, cs[11], zs), cs[27]);
    const float e1 = sub_rn(dot3_chain(cs[12], b0, cs[13], b1, cs[14], zs), cs[28]);
    const float e2 = sub_rn(dot3_chain(cs[15], b0, cs[16], b1, cs[17], zs), cs[29]);
    sx = add_rn(sx, dot3_chain(cs[18], e0, cs[21], e1, cs[24], e2));
    sy = add_rn(sy, dot3_chain(cs[19], e0, cs[22], e1, cs[25], e2));
    sz = add_rn(sz, dot3_chain(cs[20], e0, cs[23], e1, cs[26], e2));
    ++nv;
  }
  const float cnt = (float)(nv + 1);
  float* o = pts + ((size_t)r * hw + p) * 3;
  __builtin_nontemporal_store(div_rn(sx, cnt), o);
  __builtin_nontemporal_store(div_rn(sy, cnt), o + 1);
  __builtin_nontemporal_store(div_rn(sz, cnt), o + 2);
  __builtin_nontemporal_store(nv, n_valid + (size_t)r * hw + p);
}

// ---- compaction --------------------------------------------------------------------------------------------------------------

// keep mask + kept pixels per tile (tile = kTile consecutive pixels of one view; tiles never straddle views)
__global__ __launch_bounds__(kTile) void fusion_compact_count_kernel(const int* __restrict__ n_valid, int hw, int tiles_per_view,
                                                                      int thresh, unsigned char* __restrict__ all_valid,
                                                                      int* __restrict__ tile_count) {
  __shared__ int wave_cnt[kTile / 64];
  const int r = blockIdx.x / tiles_per_view;
  const int p = (blockIdx.x - r * tiles_per_view) * kTile + (int)threadIdx.x;
  bool keep = false;
  if (p < hw) {
    keep = n_valid[(size_t)r * hw + p] >= thresh;
    all_valid[(size_t)r * hw + p] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one workgroup: exclusive scan of the tile counts (each thread a contiguous chunk), then per-view offsets / counts / total
__global__ __launch_bounds__(1024) void fusion_compact_scan_kernel(const int* __restrict__ tile_count, int n_tiles, int n_ref,
                                                                    int tiles_per_view, int* __restrict__ tile_ofs,
                                                                    int* __restrict__ view_count, int* __restrict__ view_ofs,
                                                                    int* __restrict__ total) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int chunk = (n_tiles + 1023) / 1024;
  const int b = t * chunk, e = min(b + chunk, n_tiles);
  int sum = 0;
  for (int i = b; i < e; ++i) sum += tile_count[i];
  part[t] = sum;
  __syncthreads();
  for (int step = 1; step < 1024; step <<= 1) {          // Hillis-Steele inclusive scan
    const int add = t >= step ? part[t - step] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int i = b; i < e; ++i) {
    tile_ofs[i] = run;
    run += tile_count[i];
  }
  const int all = part[1023];
  __syncthreads();                                       // tile_ofs written by this workgroup is visible to it below
  for (int v = t; v <= n_ref; v += 1024) {
    const int o = v < n_ref ? tile_ofs[v * tiles_per_view] : all;
    view_ofs[v] = o;
    if (v < n_ref) view_count[v] = (v + 1 < n_ref ? tile_ofs[(v + 1) * tiles_per_view] : all) - o;
  }
  if (t == 0) *total = all;
}

// ordered scatter: rank of a kept pixel = tile offset + kept pixels before it in the tile.  WORDS = 4-byte words per colour
// (0: copy px_bytes single bytes)
template <int WORDS>
__global__ __launch_bounds__(kTile) void fusion_compact_scatter_kernel(const int* __restrict__ n_valid, const float* __restrict__ pts,
                                                                        const unsigned char* __restrict__ images, int px_bytes, int hw,
                                                                        int tiles_per_view, int thresh, const int* __restrict__ tile_ofs,
                                                                        float* __restrict__ out_pts, unsigned char* __restrict__ out_rgb) {
  __shared__ int wave_cnt[kTile / 64];
  const int r = blockIdx.x / tiles_per_view;
  const int p = (blockIdx.x - r * tiles_per_view) * kTile + (int)threadIdx.x;
  const size_t e = (size_t)r * hw + p;
  const bool keep = p < hw && n_valid[e] >= thresh;
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wave_cnt[wv] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int rank = tile_ofs[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int i = 0; i < wv; ++i) rank += wave_cnt[i];
  out_pts[(size_t)rank * 3 + 0] = pts[e * 3 + 0];
  out_pts[(size_t)rank * 3 + 1] = pts[e * 3 + 1];
  out_pts[(size_t)rank * 3 + 2] = pts[e * 3 + 2];
  if (images) {
    if (WORDS > 0) {
      const unsigned* src = reinterpret_cast<const unsigned*>(images) + e * WORDS;
      unsigned* dst = reinterpret_cast<unsigned*>(out_rgb) + (size_t)rank * WORDS;
#pragma unroll
      for (int i = 0; i < WORDS; ++i) dst[i] = src[i];
    } else {
      for (int i = 0; i < px_bytes; ++i) out_rgb[(size_t)rank * px_bytes + i] = images[e * px_bytes + i];
    }
  }
}

// workspace: [source lists: ref_img n_img | edge_ofs n_img + 1 | edge_src n_img^2][tile_count][tile_ofs]
inline size_t list_bytes(int n_img) { return v3d::align_up(((size_t)n_img * 2 + 1 + (size_t)n_img * n_img) * 4, 256); }
inline int tiles_of(int h, int w) { return (h * w + kTile - 1) / kTile; }
inline size_t tile_bytes(int n_img, int h, int w) { return v3d::align_up((size_t)n_img * tiles_of(h, w) * 4, 256); }

int check_sizes(const char* fn, int n_img, int n_ref, int h, int w) {
  V3D_REQUIRE(n_img >= 1 && n_img <= 4096 && n_ref >= 1 && n_ref <= n_img, V3D_ERR_BAD_SHAPE,
              "%s: n_img=%d n_ref=%d (1 <= n_ref <= n_img <= 4096)", fn, n_img, n_ref);
  V3D_REQUIRE(h >= 2 && w >= 2, V3D_ERR_BAD_SHAPE, "%s: h=%d w=%d (the coordinate normalisation divides by h-1 and w-1)", fn, h, w);
  V3D_REQUIRE((long long)h * w <= (1ll << 24) && (long long)n_img * h * w < (1ll << 31) / 3, V3D_ERR_BAD_SHAPE,
              "%s: %d maps of %d x %d exceed the 32-bit index range", fn, n_img, h, w);
  return V3D_OK;
}

}  // namespace

extern "C" size_t v3d_fusion_workspace_bytes(int n_img, int h, int w) {
  if (n_img < 1 || n_img > 4096 || h < 2 || w < 2 || (long long)h * w > (1ll << 24)) return 0;
  return list_bytes(n_img) + 2 * tile_bytes(n_img, h, w);
}

extern "C" int v3d_fuse_depths_f32(const float* depths, const float* cams, int n_img, int h, int w, const int32_t* ref_img_host,
                                   int n_ref, const int32_t* edge_ofs_host, const int32_t* edge_src_host, double z_thresh,
                                   float* pts, int32_t* n_valid, void* workspace, size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(depths && cams && pts && n_valid && workspace, V3D_ERR_BAD_ARG, "v3d_fuse_depths_f32: null argument");
  if (int rc = check_sizes("v3d_fuse_depths_f32", n_img, n_ref, h, w)) return rc;
  V3D_REQUIRE((edge_ofs_host == nullptr) == (edge_src_host == nullptr), V3D_ERR_BAD_ARG,
              "v3d_fuse_depths_f32: edge_ofs_host and edge_src_host go together");
  V3D_REQUIRE(ref_img_host || n_ref == n_img, V3D_ERR_BAD_ARG, "v3d_fuse_depths_f32: n_ref=%d != n_img=%d needs ref_img_host", n_ref, n_img);
  V3D_REQUIRE(z_thresh >= 0.0, V3D_ERR_BAD_ARG, "v3d_fuse_depths_f32: z_thresh=%g", z_thresh);
  V3D_REQUIRE(workspace_bytes >= v3d_fusion_workspace_bytes(n_img, h, w), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_fuse_depths_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int* d_ref = (int*)workspace;
  int* d_ofs = d_ref + n_img;
  int* d_src = d_ofs + n_img + 1;
  if (ref_img_host) {
    for (int r = 0; r < n_ref; ++r)
      V3D_REQUIRE(ref_img_host[r] >= 0 && ref_img_host[r] < n_img, V3D_ERR_BAD_ARG,
                  "v3d_fuse_depths_f32: reference index %d (entry %d) out of range [0, %d)", ref_img_host[r], r, n_img);
    V3D_CHECK_HIP(hipMemcpyAsync(d_ref, ref_img_host, (size_t)n_ref * 4, hipMemcpyHostToDevice, s));
  }
  if (edge_ofs_host) {
    V3D_REQUIRE(edge_ofs_host[0] == 0, V3D_ERR_BAD_ARG, "v3d_fuse_depths_f32: edge_ofs[0] = %d", edge_ofs_host[0]);
    for (int r = 0; r < n_ref; ++r)
      V3D_REQUIRE(edge_ofs_host[r + 1] >= edge_ofs_host[r], V3D_ERR_BAD_ARG, "v3d_fuse_depths_f32: edge_ofs decreases at %d", r);
    const int n_edges = edge_ofs_host[n_ref];
    V3D_REQUIRE((long long)n_edges <= (long long)n_img * n_img, V3D_ERR_BAD_ARG,
                "v3d_fuse_depths_f32: %d edges (at most n_img^2 = %d)", n_edges, n_img * n_img);
    for (int j = 0; j < n_edges; ++j)
      V3D_REQUIRE(edge_src_host[j] >= 0 && edge_src_host[j] < n_img, V3D_ERR_BAD_ARG,
                  "v3d_fuse_depths_f32: source index %d (edge %d) out of range [0, %d)", edge_src_host[j], j, n_img);
    V3D_CHECK_HIP(hipMemcpyAsync(d_ofs, edge_ofs_host, (size_t)(n_ref + 1) * 4, hipMemcpyHostToDevice, s));
    if (n_edges) V3D_CHECK_HIP(hipMemcpyAsync(d_src, edge_src_host, (size_t)n_edges * 4, hipMemcpyHostToDevice, s));
  }
  const int tpv = tiles_of(h, w);
  const long long grid = (long long)n_ref * tpv;
  v3d::TimedScope ts("fuse_depths", s);
  fuse_depths_kernel<<<(unsigned)grid, kTile, 0, s>>>(depths, cams, ref_img_host ? d_ref : nullptr, edge_ofs_host ? d_ofs : nullptr,
                                                      edge_ofs_host ? d_src : nullptr, n_img, h * w, w, h, tpv,
                                                      v3d::magic_u32((unsigned long long)grid, (unsigned)tpv), (float)z_thresh, pts,
                                                      n_valid);
  V3D_CHECK_LAUNCH("fuse_depths_kernel");
  return V3D_OK;
}

extern "C" int v3d_fusion_compact(const int32_t* n_valid, const float* pts, const void* images, int px_bytes, int n_ref, int h,
                                  int w, int n_consistent_thresh, uint8_t* all_valid, int32_t* view_count, int32_t* view_ofs,
                                  float* out_pts, void* out_rgb, int32_t* total, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  V3D_REQUIRE(n_valid && pts && all_valid && view_count && view_ofs && out_pts && total && workspace, V3D_ERR_BAD_ARG,
              "v3d_fusion_compact: null argument");
  V3D_REQUIRE((images == nullptr) == (out_rgb == nullptr), V3D_ERR_BAD_ARG, "v3d_fusion_compact: images and out_rgb go together");
  V3D_REQUIRE(!images || (px_bytes >= 1 && px_bytes <= 64), V3D_ERR_BAD_ARG, "v3d_fusion_compact: px_bytes=%d (1..64)", px_bytes);
  if (int rc = check_sizes("v3d_fusion_compact", n_ref, n_ref, h, w)) return rc;
  V3D_REQUIRE(workspace_bytes >= v3d_fusion_workspace_bytes(n_ref, h, w), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_fusion_compact: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int tpv = tiles_of(h, w), n_tiles = n_ref * tpv, hw = h * w;
  int* tile_count = (int*)((char*)workspace + list_bytes(n_ref));
  int* tile_ofs = (int*)((char*)tile_count + tile_bytes(n_ref, h, w));
  v3d::TimedScope ts("fusion_compact", s);
  fusion_compact_count_kernel<<<n_tiles, kTile, 0, s>>>(n_valid, hw, tpv, n_consistent_thresh, all_valid, tile_count);
  V3D_CHECK_LAUNCH("fusion_compact_count_kernel");
  fusion_compact_scan_kernel<<<1, 1024, 0, s>>>(tile_count, n_tiles, n_ref, tpv, tile_ofs, view_count, view_ofs, total);
  V3D_CHECK_LAUNCH("fusion_compact_scan_kernel");
  const unsigned char* img = (const unsigned char*)images;
  unsigned char* rgb = (unsigned char*)out_rgb;
  const bool words = images && px_bytes == 12 && ((uintptr_t)images % 4 == 0) && ((uintptr_t)out_rgb % 4 == 0);
  if (words)
    fusion_compact_scatter_kernel<3><<<n_tiles, kTile, 0, s>>>(n_valid, pts, img, px_bytes, hw, tpv, n_consistent_thresh, tile_ofs,
                                                               out_pts, rgb);
  else
    fusion_compact_scatter_kernel<0><<<n_tiles, kTile, 0, s>>>(n_valid, pts, img, px_bytes, hw, tpv, n_consistent_thresh, tile_ofs,
                                                               out_pts, rgb);
  V3D_CHECK_LAUNCH("fusion_compact_scatter_kernel");
  return V3D_OK;
}
