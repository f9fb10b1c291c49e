// What the translation units of the regulariser share (costreg.hip is the map of the family): the weight handle, the layer
// table, the launch parameters and lane helpers common to several kernel families, and every family's launcher and packer.
#pragma once
#include "bf16_split.h"
#include "v3d_common.h"

struct v3d_costreg_weights {
  int in_channels, base;
  float* dev;                 // one allocation holding everything below
  size_t wp_ofs[10], bias_ofs[10], prob_w2_ofs, prob_b_ofs, c0bf_ofs, c0f32_ofs, cgbf_ofs[7], dgbf_ofs[2], c9bf_ofs, c9f32_ofs, total;
};

namespace v3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// CostRegNet(32, 8), mvsnet.py:133-163: conv0..conv6 (k3 p1, stride 1 or 2), conv7..conv9 (k3 s2 p1 output_padding-1 transposed
// convolutions); conv0 has `in_channels` (32 or 16) inputs
struct LayerDesc { int cin, cout; bool deconv; };
constexpr LayerDesc kLayers[10] = {{32, 8, false},  {8, 16, false},  {16, 16, false}, {16, 32, false}, {32, 32, false},
                                   {32, 64, false}, {64, 64, false}, {64, 32, true},  {32, 16, true},  {16, 8, true}};

// outputs of the split-bf16 kernels of conv1..conv8: fp32 [n, C, D, H, W] (per-layer entry point) / the split channel-last
// layout [n][C/8 groups][hi, lo][D][H][W][8 bf16] (the chain)
enum { kOutF32 = 1, kOutSplit = 2 };

// launch parameters of conv3d_mfma_kernel (costreg_fp32.hip) and conv0_bf16x2_kernel (costreg_conv0.hip)
struct ConvParams {
  const float* in;
  const float* wp;     // packed A fragments
  const float* bias;   // [COUT]
  const float* skip;   // [n, COUT, Do, Ho, Wo] or null
  float* out;
  int n, Di, Hi, Wi, Do, Ho, Wo, ntz, nty, ntx;
  int relu;
  int zy_order;        // tile order inside a view: 0 = x, y, z (z slowest), 1 = x, z, y (conv0 on large planes, see tile_order())
};

// The workgroups resident on an XCD (64 tiles of conv0 / conv9+prob) should be neighbours in the directions with the most
// halo: a 4 x 8 x 28 tile re-reads 50 % in z, 25 % in y, 7 % in x.  With x, y, z order they cover several whole z slabs when
// a slab is small (cfg2: 2 x 7 = 14 tiles) but only part of one when it is large (cfg5: 6 x 15 = 90 tiles: conv0 fetched
// 1.5x its input); then x, z, y order puts z neighbours side by side.
inline int tile_order(int ntx, int nty) {
#ifdef V3D_TILE_ORDER_XYZ      // developer A/B
  return 0;
#else
  return ntx * nty > 32 ? 1 : 0;
#endif
}

// Tile grid of a split-bf16 kernel that finds its tile with host magic numbers: the tile counts of a tD x tH x tW volume cut
// into td x th x tw tiles, the workgroup count, and v3d::magic_u32() of ntx and of the two counts divided after it (y then z,
// or z then y with zy_order; 0: divide).  These kernels address one view's tensors with 32-bit slot offsets built from
// 24-bit multiplies: the volume vD x vH x vW they index must stay below max_voxels (slot bytes x planes x voxels < 4 GB).
struct TileGrid { int ntz, nty, ntx; unsigned m_tx, m_t1, m_t2; long long blocks; };
inline int tile_grid(const char* name, int n, int tD, int tH, int tW, int td, int th, int tw, int zy_order, int vD, int vH, int vW,
                     long long max_voxels, TileGrid* g) {
  g->ntz = (tD + td - 1) / td; g->nty = (tH + th - 1) / th; g->ntx = (tW + tw - 1) / tw;
  g->blocks = (long long)n * g->ntz * g->nty * g->ntx;
  V3D_REQUIRE(g->blocks > 0 && g->blocks < (1ll << 31), V3D_ERR_BAD_SHAPE, "%s: bad grid", name);
  V3D_REQUIRE(vD < (1 << 12) && vH < (1 << 12) && vW < (1 << 12) && (long long)vD * vH * vW < max_voxels, V3D_ERR_BAD_SHAPE,
              "%s: volume %d x %d x %d too large for 32-bit slot offsets", name, vD, vH, vW);
  const int d1 = zy_order ? g->ntz : g->nty, d2 = zy_order ? g->nty : g->ntz;
  g->m_tx = magic_u32((unsigned long long)g->blocks, (unsigned)g->ntx);
  g->m_t1 = magic_u32((unsigned long long)g->blocks / g->ntx + 1, (unsigned)d1);
  g->m_t2 = magic_u32((unsigned long long)g->blocks / g->ntx / d1 + 1, (unsigned)d2);
  return V3D_OK;
}

// cond ? a : b as a bit select (v_bfi_b32): written with ?: on two arrays the compiler turns the pair into a private array
// indexed by the lane, i.e. scratch memory and a vector load the epilogue then has to wait for.
__device__ __forceinline__ float lane_select(int cond, float a, float b) {
  const unsigned m = 0u - (unsigned)(cond != 0);
  return __uint_as_float((__float_as_uint(a) & m) | (__float_as_uint(b) & ~m));
}

// words from a lane's hi words to its lo words in a [hi, lo][lane 64][4 words] fragment block (v3d::split_bf16x8)
constexpr int kLoWords = 64 * 4;

// ---- costreg_fp32.hip: the exact-fp32 per-layer kernels.  `w` = the BN-folded weights in the layout of the layer's conv_w.
size_t tile_image_floats(int layer, int in_channels);
void pack_tile_image(int layer, int in_channels, const float* w, float* wp);
int launch_conv_fp32(int layer, int in_channels, const float* in, const float* wp, const float* bias, const float* skip, float* out,
                     int n, int Di, int Hi, int Wi, hipStream_t s);

// ---- costreg_conv0.hip: conv0 as a tile kernel on split-bf16 matrix cores, and the two weight images of conv0z.hip
constexpr size_t kConv0SplitFloats = (size_t)4 * 9 * 2 * kLoWords, kConv0F32Floats = (size_t)4 * 9 * 8 * 64;
void pack_conv0_split(const float* w, int in_channels, unsigned* wb);
void pack_conv0_f32(const float* w, int in_channels, float* wf);
int launch_conv0_bf16(const float* in, const float* wbf, const float* bias, const float* skip, float* out, int n, int Di, int Hi,
                      int Wi, hipStream_t s);

// ---- costreg_convg.hip: conv1..conv6 / conv7, conv8 on split-bf16 matrix cores.  `layer` 1..8, input in the split layout;
// out = kOutF32: `dst` = fp32 [n, Cout, Do, Ho, Wo], `skip` (conv7, conv8) fp32 of the same shape; out = kOutSplit: `dst` and
// `skip` in the split layout.
void pack_convg(const float* w, int cin, int cout, unsigned* wb);
void pack_deconvg(const float* w, int cin, int cout, unsigned* wb);
int launch_split_layer(int layer, int out, const void* in, const float* wbf, const float* bias, const void* skip, void* dst, int n,
                       int Di, int Hi, int Wi, hipStream_t s);
// fp32 [n, C, D, H, W] -> the split layout; plane = D * H * W, total = n * (C / 8) * plane
int launch_encode_split(const float* in, void* out, int C, size_t plane, size_t total, hipStream_t s);

// ---- costreg_conv9.hip: conv9 + conv0 skip + the prob conv in one tile kernel (split-bf16 or exact-fp32 operands)
constexpr size_t kConv9SplitFloats = (size_t)9 * 2 * kLoWords, kConv9F32Floats = (size_t)9 * 64 * 8;
void pack_conv9(const float* w, unsigned* wb, float* wf);
void pack_prob(const float* prob_w, float* out);
int launch_conv9_prob(bool f32, const v3d_costreg_weights* h, const float* u8, const float* c0, float* xreg, int n, int D, int H, int W,
                      hipStream_t s);

// conv0 of CostRegNet as a depth march (conv0z.hip).  f32 = false: split variance volume [n][4][hi, lo][D][H][W] -> split
// activation [n][hi, lo][D][H][W] (16-byte slots of 8 bf16), `wimg` = the split-bf16 weight image of conv0 (pack_conv0_split).
// f32 = true: fp32 channel-last volume [n][4][2 halves][D][H][W] (16-byte slots of 4 floats) -> fp32 [n, 8, D, H, W],
// `wimg` = the fp32 fragment image (pack_conv0_f32).
int launch_conv0z(bool f32, const void* in, const float* wimg, const float* bias, void* out, int n, int D, int H, int W,
                  hipStream_t s);

// conv1 + conv2 of CostRegNet as one depth march (conv12z.hip, experiment): conv0 output [n][hi, lo][D][H][W] (split layout)
// -> conv2 output [n][2 groups][hi, lo][D2][H2][W2]; `w1` / `w2` = the split-bf16 images of conv1 / conv2 (pack_convg)
int launch_conv12z(const void* c0_split, const float* w1, const float* w2, const float* b1, const float* b2, void* out_split,
                   int n, int D, int H, int W, hipStream_t s);

// confidence.hip: the soft-argmin x_reg [n, D, H, W] -> depth [n, H, W], and the one that also writes the confidence of its own
// depth (prob [n, H, W]); both walk the planes with the same function, so the depth has the same bits
int launch_soft_argmin(const float* xreg, const float* depth_vals, float* depth, int n, int D, int H, int W, hipStream_t s);
int launch_soft_argmin_prob(const float* xreg, const float* depth_vals, float* depth, float* prob, double depth_start,
                            double depth_interval, int n, int D, int H, int W, hipStream_t s);

}  // namespace v3d
