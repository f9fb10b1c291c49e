// Triangle meshes from TSDF volumes: marching cubes with the project's own case table (mc_table.h, generated from a rule by
// scripts/gen_mc_table.py) and the rules mv3d/eval/tsdf_atlas.py applies around its marching-cubes call -- TSDF.get_mesh
// (:161-253: clamp, empty-mesh rule, the -1 / +1 "bad vertex" rule, colour lookup at round(vertex), world transform, removal of
// bad vertices with renumbering) and the tsdf_point_cloud attribute of get_tsdf (:465-481).
//
//   mc_classify_kernel   one thread per voxel, lanes along z (the fastest axis): the sign of the clamped value, which of the up to
//                        three edges the voxel owns (+x, +y, +z, inside the volume) change sign, and -- get_mesh mode -- which of
//                        those vertices survive the bad-vertex rule.  One status byte per voxel.
//   mc_tricount_kernel   one thread per cell (= the voxel of its corner 0): the case from the eight status bytes, the number of
//                        table triangles whose three vertices all survive.  One byte per voxel.
//   mc_totals_*          exact 64-bit totals of both counts, minimum / maximum of the clamped volume (empty-mesh rule): a fixed
//                        two-stage tree.  The totals land in two device words.
//   rocPRIM exclusive scans of both counts (32-bit: the totals are checked to be < 2^31 first).
//   mc_emit_*            vertices in (voxel flat index, axis) order, triangles in (cell flat index, table) order with indices into
//                        the FINAL vertex numbering: the offset of the owning voxel from the scan + the rank of the axis among the
//                        surviving vertices of that voxel.
// No atomics, no LDS outside the totals tree, no scratch (build-time ISA guard): the output is a function of the volume alone and
// repeated launches are bit-identical.
//
// Arithmetic (all fp32, DESIGN.md §2 for the convention): t = va / (va - vb), one rounded subtraction and one IEEE division;
// index coordinate = fl(float(i) + t); world = fl(fl(index * voxel_size) + origin), two roundings as NumPy's separate multiply and
// add give on the reference's float32 vertex array.  The bad-vertex cell and the colour voxel come from that fp32 index coordinate
// (floor / round-half-even), as the reference takes them: t can round to 1, and t = 0.5 is a tie.
//
// A corner is inside iff its clamped value is < 0: NaN and -0.0 are outside.  The clamp keeps a NaN a NaN, as torch.clamp does.
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "v3d_common.h"

#define V3D_MC_TABLE_DECL static __device__ __attribute__((aligned(16)))      // a row is one 16-byte load
#include "mc_table.h"

namespace {

using v3d::add_rn;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kTile = 256;
constexpr int kRedBlocks = 256;
constexpr unsigned kInside = 64u;          // status byte: bits 0..2 sign change along x, y, z; bits 3..5 the vertex survives; bit 6 inside

struct McMeta {           // device-resident state of a count call, read by the emit kernels
  int n_verts;
  int n_tris;
  int empty;              // the reference's empty-mesh rule applies
  int overflow;           // a total reached 2^31
};

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

__device__ __forceinline__ float clamp1(float v) { return v < -1.f ? -1.f : (v > 1.f ? 1.f : v); }

// a floored / rounded index coordinate -> voxel index inside [0, n): NaN and negatives give 0
__device__ __forceinline__ int clip_index(float f, int n) {
  f = f >= 0.f ? f : 0.f;
  f = fminf(f, (float)(n - 1));
  const int i = (int)f;
  return i < n - 1 ? i : n - 1;
}

struct Dims { int nx, ny, nz, n_vox; };

// among the eight clamped values at floor(vertex) + {0, 1}^3 (clipped to the volume) one is +1 and one is -1
__device__ __forceinline__ bool bad_vertex(const float* __restrict__ tsdf, const Dims d, float cx, float cy, float cz) {
  const int x0 = clip_index(floorf(cx), d.nx), y0 = clip_index(floorf(cy), d.ny), z0 = clip_index(floorf(cz), d.nz);
  const int x1 = min(x0 + 1, d.nx - 1), y1 = min(y0 + 1, d.ny - 1), z1 = min(z0 + 1, d.nz - 1);
  bool hi = false, lo = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int x = (c & 4) ? x1 : x0, y = (c & 2) ? y1 : y0, z = (c & 1) ? z1 : z0;
    const float v = clamp1(tsdf[((size_t)x * d.ny + y) * d.nz + z]);
    hi = hi || v == 1.f;
    lo = lo || v == -1.f;
  }
  return hi && lo;
}

template <bool MESH>
__global__ __launch_bounds__(kTile) void mc_classify_kernel(const float* __restrict__ tsdf, const Dims d,
                                                             unsigned char* __restrict__ mask) {
  const int i = (int)blockIdx.x * kTile + (int)threadIdx.x;
  if (i >= d.n_vox) return;
  const int xy = i / d.nz, z = i - xy * d.nz;
  const int x = xy / d.ny, y = xy - x * d.ny;
  const float v = clamp1(tsdf[i]);
  const bool in = v < 0.f;
  const float fx = (float)x, fy = (float)y, fz = (float)z;
  unsigned m = in ? kInside : 0u;
  if (x + 1 < d.nx) {
    const float vb = clamp1(tsdf[(size_t)i + (size_t)d.ny * d.nz]);
    if ((vb < 0.f) != in) {
      m |= 1u;
      if (!MESH || !bad_vertex(tsdf, d, add_rn(fx, div_rn(v, sub_rn(v, vb))), fy, fz)) m |= 8u;
    }
  }
  if (y + 1 < d.ny) {
    const float vb = clamp1(tsdf[(size_t)i + d.nz]);
    if ((vb < 0.f) != in) {
      m |= 2u;
      if (!MESH || !bad_vertex(tsdf, d, fx, add_rn(fy, div_rn(v, sub_rn(v, vb))), fz)) m |= 16u;
    }
  }
  if (z + 1 < d.nz) {
    const float vb = clamp1(tsdf[(size_t)i + 1]);
    if ((vb < 0.f) != in) {
      m |= 4u;
      if (!MESH || !bad_vertex(tsdf, d, fx, fy, add_rn(fz, div_rn(v, sub_rn(v, vb))))) m |= 32u;
    }
  }
  mask[i] = (unsigned char)m;
}

// The eight status bytes of a cell (byte c = corner c: x = c & 1, y = (c >> 1) & 1, z = (c >> 2) & 1) -> the case index and,
// bit e, whether the vertex on cell edge e = 4 axis + u + 2 v survives.
__device__ __forceinline__ unsigned long long cell_bytes(const unsigned char* __restrict__ mask, size_t i, size_t sx, size_t sy) {
  unsigned long long mm = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const size_t j = i + ((c & 1) ? sx : 0) + ((c & 2) ? sy : 0) + ((c & 4) ? 1 : 0);
    mm |= (unsigned long long)mask[j] << (8 * c);
  }
  return mm;
}

__device__ __forceinline__ void cell_state(unsigned long long mm, unsigned& cas, unsigned& kept) {
  cas = 0;
  kept = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cas |= (unsigned)((mm >> (8 * c + 6)) & 1ull) << c;
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
    const int c = a == 0 ? ((u << 1) | (v << 2)) : (a == 1 ? (u | (v << 2)) : (u | (v << 1)));     // the owning corner
    kept |= (unsigned)((mm >> (8 * c + 3 + a)) & 1ull) << e;
  }
}

// triangle k (0..4) of a table row loaded as four 32-bit words
__device__ __forceinline__ unsigned row_tri(const uint4 w, int k) {
  return k == 0 ? w.x >> 16 : (k == 1 ? w.y & 0xffffu : (k == 2 ? w.y >> 16 : (k == 3 ? w.z & 0xffffu : w.z >> 16)));
}
__device__ __forceinline__ bool tri_kept(unsigned tri, unsigned kept) {
  return ((kept >> (tri & 15u)) & (kept >> ((tri >> 4) & 15u)) & (kept >> ((tri >> 8) & 15u)) & 1u) != 0u;
}

__global__ __launch_bounds__(kTile) void mc_tricount_kernel(const unsigned char* __restrict__ mask, const Dims d,
                                                             unsigned char* __restrict__ tcnt) {
  const int i = (int)blockIdx.x * kTile + (int)threadIdx.x;
  if (i >= d.n_vox) return;
  const int xy = i / d.nz, z = i - xy * d.nz;
  const int x = xy / d.ny, y = xy - x * d.ny;
  unsigned n = 0;
  if (x + 1 < d.nx && y + 1 < d.ny && z + 1 < d.nz) {
    unsigned cas, kept;
    cell_state(cell_bytes(mask, (size_t)i, (size_t)d.ny * d.nz, (size_t)d.nz), cas, kept);
    if (cas != 0u && cas != 255u) {
      const uint4 w = *reinterpret_cast<const uint4*>(&kMcTable[cas][0]);
      const unsigned ntri = w.x & 0xffffu;
#pragma unroll
      for (int k = 0; k < 5; ++k)
        if ((unsigned)k < ntri && tri_kept(row_tri(w, k), kept)) ++n;
    }
  }
  tcnt[i] = (unsigned char)n;
}

__device__ __forceinline__ unsigned kept_count(unsigned m) { return (unsigned)__popc((m >> 3) & 7u); }

struct KeptCount {
  __device__ __host__ unsigned operator()(unsigned char m) const { return (unsigned)(((m >> 3) & 1) + ((m >> 4) & 1) + ((m >> 5) & 1)); }
};
struct ByteCount {
  __device__ __host__ unsigned operator()(unsigned char m) const { return (unsigned)m; }
};

// stage 1 of the totals: block b sums its grid-stride share of both counts in 64 bits and takes the minimum / maximum of the
// clamped volume; the tree in LDS has a fixed shape
__global__ __launch_bounds__(256) void mc_totals_partial_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ mask,
                                                                 const unsigned char* __restrict__ tcnt, int n_vox,
                                                                 unsigned long long* __restrict__ part_n, float* __restrict__ part_f) {
  unsigned long long nv = 0, nt = 0;
  float lo = INFINITY, hi = -INFINITY, nan = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_vox; i += (long long)kRedBlocks * 256) {
    nv += kept_count(mask[i]);
    if (tcnt) nt += tcnt[i];
    const float v = clamp1(tsdf[i]);
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    if (v != v) nan = 1.f;
  }
  __shared__ unsigned long long sn[2][256];
  __shared__ float sf[3][256];
  sn[0][threadIdx.x] = nv;
  sn[1][threadIdx.x] = nt;
  sf[0][threadIdx.x] = lo;
  sf[1][threadIdx.x] = hi;
  sf[2][threadIdx.x] = nan;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sn[0][threadIdx.x] += sn[0][threadIdx.x + o];
      sn[1][threadIdx.x] += sn[1][threadIdx.x + o];
      sf[0][threadIdx.x] = fminf(sf[0][threadIdx.x], sf[0][threadIdx.x + o]);
      sf[1][threadIdx.x] = fmaxf(sf[1][threadIdx.x], sf[1][threadIdx.x + o]);
      sf[2][threadIdx.x] = fmaxf(sf[2][threadIdx.x], sf[2][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) part_n[blockIdx.x * 2 + threadIdx.x] = sn[threadIdx.x][0];
  if (threadIdx.x < 3) part_f[blockIdx.x * 3 + threadIdx.x] = sf[threadIdx.x][0];
}

// stage 2: one workgroup over the partials -> the meta record and the two count words.  Empty-mesh rule (get_mesh mode): the
// minimum of the clamped volume is >= 0 or the maximum is <= 0; with a NaN in the volume NumPy's min / max are NaN and both
// comparisons fail, so the rule does not apply.
__global__ __launch_bounds__(256) void mc_totals_finish_kernel(const unsigned long long* __restrict__ part_n, const float* __restrict__ part_f,
                                                                int nblocks, int mesh_mode, McMeta* __restrict__ meta,
                                                                int* __restrict__ counts) {
  __shared__ unsigned long long sn[2][256];
  __shared__ float sf[3][256];
  const bool on = (int)threadIdx.x < nblocks;
  sn[0][threadIdx.x] = on ? part_n[threadIdx.x * 2] : 0ull;
  sn[1][threadIdx.x] = on ? part_n[threadIdx.x * 2 + 1] : 0ull;
  sf[0][threadIdx.x] = on ? part_f[threadIdx.x * 3] : INFINITY;
  sf[1][threadIdx.x] = on ? part_f[threadIdx.x * 3 + 1] : -INFINITY;
  sf[2][threadIdx.x] = on ? part_f[threadIdx.x * 3 + 2] : 0.f;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      sn[0][threadIdx.x] += sn[0][threadIdx.x + o];
      sn[1][threadIdx.x] += sn[1][threadIdx.x + o];
      sf[0][threadIdx.x] = fminf(sf[0][threadIdx.x], sf[0][threadIdx.x + o]);
      sf[1][threadIdx.x] = fmaxf(sf[1][threadIdx.x], sf[1][threadIdx.x + o]);
      sf[2][threadIdx.x] = fmaxf(sf[2][threadIdx.x], sf[2][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const bool empty = mesh_mode && sf[2][0] == 0.f && (sf[0][0] >= 0.f || sf[1][0] <= 0.f);
  const bool overflow = !empty && (sn[0][0] >= (1ull << 31) || sn[1][0] >= (1ull << 31));
  meta->empty = empty ? 1 : 0;
  meta->overflow = overflow ? 1 : 0;
  meta->n_verts = (empty || overflow) ? 0 : (int)sn[0][0];
  meta->n_tris = (empty || overflow) ? 0 : (int)sn[1][0];
  counts[0] = overflow ? -1 : meta->n_verts;
  counts[1] = overflow ? -1 : meta->n_tris;
}

// MESH: colours clamped to [0, 255], truncated, stored in channel order [2, 1, 0]; else floor, channel order [0, 1, 2]
template <bool MESH>
__device__ __forceinline__ void emit_vertex(const Dims d, const float* __restrict__ color, float cx, float cy, float cz, float vs,
                                            float ox, float oy, float oz, size_t row, float* __restrict__ verts,
                                            unsigned char* __restrict__ colors) {
  verts[row * 3 + 0] = add_rn(mul_rn(cx, vs), ox);
  verts[row * 3 + 1] = add_rn(mul_rn(cy, vs), oy);
  verts[row * 3 + 2] = add_rn(mul_rn(cz, vs), oz);
  if (color) {
    const int ix = clip_index(rintf(cx), d.nx), iy = clip_index(rintf(cy), d.ny), iz = clip_index(rintf(cz), d.nz);
    const size_t j = ((size_t)ix * d.ny + iy) * d.nz + iz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = color[(size_t)c * d.n_vox + j];
      if (MESH)
        colors[row * 3 + (2 - c)] = (unsigned char)(int)(v >= 0.f ? (v > 255.f ? 255.f : v) : 0.f);      // a NaN gives 0
      else
        colors[row * 3 + c] = (unsigned char)(int)floorf(v);
    }
  }
}

template <bool MESH>
__global__ __launch_bounds__(kTile) void mc_emit_vertices_kernel(const float* __restrict__ tsdf, const float* __restrict__ color,
                                                                  const Dims d, float vs, float ox, float oy, float oz,
                                                                  const unsigned char* __restrict__ mask, const unsigned* __restrict__ vofs,
                                                                  const McMeta* __restrict__ meta, float* __restrict__ verts,
                                                                  unsigned char* __restrict__ colors, int v_cap) {
  const int i = (int)blockIdx.x * kTile + (int)threadIdx.x;
  if (i >= d.n_vox || meta->empty || meta->overflow) return;
  const unsigned m = mask[i];
  if (((m >> 3) & 7u) == 0u) return;
  const int xy = i / d.nz, z = i - xy * d.nz;
  const int x = xy / d.ny, y = xy - x * d.ny;
  const float fx = (float)x, fy = (float)y, fz = (float)z;
  const float v = clamp1(tsdf[i]);
  size_t row = vofs[i];
  // the bounds tests only matter for a workspace that no count call filled: no read leaves the volume even then
  if ((m & 8u) && x + 1 < d.nx) {
    const float vb = clamp1(tsdf[(size_t)i + (size_t)d.ny * d.nz]);
    if (row < (size_t)v_cap)
      emit_vertex<MESH>(d, color, add_rn(fx, div_rn(v, sub_rn(v, vb))), fy, fz, vs, ox, oy, oz, row, verts, colors);
    ++row;
  }
  if ((m & 16u) && y + 1 < d.ny) {
    const float vb = clamp1(tsdf[(size_t)i + d.nz]);
    if (row < (size_t)v_cap)
      emit_vertex<MESH>(d, color, fx, add_rn(fy, div_rn(v, sub_rn(v, vb))), fz, vs, ox, oy, oz, row, verts, colors);
    ++row;
  }
  if ((m & 32u) && z + 1 < d.nz) {
    const float vb = clamp1(tsdf[(size_t)i + 1]);
    if (row < (size_t)v_cap)
      emit_vertex<MESH>(d, color, fx, fy, add_rn(fz, div_rn(v, sub_rn(v, vb))), vs, ox, oy, oz, row, verts, colors);
  }
}

__global__ __launch_bounds__(kTile) void mc_emit_triangles_kernel(const Dims d, const unsigned char* __restrict__ mask,
                                                                   const unsigned char* __restrict__ tcnt, const unsigned* __restrict__ vofs,
                                                                   const unsigned* __restrict__ tofs, const McMeta* __restrict__ meta,
                                                                   int* __restrict__ tris, int f_cap) {
  const int i = (int)blockIdx.x * kTile + (int)threadIdx.x;
  if (i >= d.n_vox || meta->empty || meta->overflow) return;
  if (tcnt[i] == 0) return;                     // also every voxel that is not corner 0 of a cell
  const int xy = i / d.nz, z = i - xy * d.nz;
  const int x = xy / d.ny, y = xy - x * d.ny;
  if (x + 1 >= d.nx || y + 1 >= d.ny || z + 1 >= d.nz) return;      // only with a workspace that no count call filled
  const size_t sx = (size_t)d.ny * d.nz, sy = (size_t)d.nz;
  const unsigned long long mm = cell_bytes(mask, (size_t)i, sx, sy);
  unsigned cas, kept;
  cell_state(mm, cas, kept);
  const uint4 w = *reinterpret_cast<const uint4*>(&kMcTable[cas][0]);
  const unsigned ntri = w.x & 0xffffu;
  size_t row = tofs[i];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned tri = row_tri(w, k);
    if ((unsigned)k >= ntri || !tri_kept(tri, kept)) continue;
    if (row < (size_t)f_cap) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned e = (tri >> (4 * j)) & 15u;
        const unsigned a = e >> 2, u = e & 1u, v = (e >> 1) & 1u;
        const unsigned cx = a == 0u ? 0u : u, cy = a == 0u ? u : (a == 1u ? 0u : v), cz = a == 2u ? 0u : v;
        const size_t owner = (size_t)i + (cx ? sx : 0) + (cy ? sy : 0) + cz;
        const unsigned om = (unsigned)(mm >> (8u * (cx | (cy << 1) | (cz << 2)))) & 0xffu;
        const unsigned rank = (unsigned)__popc((om >> 3) & ((1u << a) - 1u));
        tris[row * 3 + j] = (int)(vofs[owner] + rank);
      }
    }
    ++row;
  }
}

struct McLayout { size_t part_n, part_f, mask, tcnt, vofs, tofs, temp, temp_bytes, total; };

McLayout mc_layout(long long n_vox) {
  McLayout l;
  const size_t m = n_vox > 0 ? (size_t)n_vox : 1;
  size_t b = 0;
  (void)rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator((const unsigned char*)nullptr, KeptCount()),
                                (unsigned*)nullptr, 0u, m, rocprim::plus<unsigned>(), (hipStream_t)0);
  l.temp_bytes = v3d::align_up(b, 256);
  size_t o = 256;
  l.part_n = o; o += v3d::align_up(kRedBlocks * 2 * sizeof(unsigned long long), 256);
  l.part_f = o; o += v3d::align_up(kRedBlocks * 3 * sizeof(float), 256);
  l.mask = o; o += v3d::align_up(m, 256);
  l.tcnt = o; o += v3d::align_up(m, 256);
  l.vofs = o; o += v3d::align_up(m * 4, 256);
  l.tofs = o; o += v3d::align_up(m * 4, 256);
  l.temp = o; o += l.temp_bytes;
  l.total = o;
  return l;
}

inline bool volume_ok(int nx, int ny, int nz) {
  return nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31);
}

}  // namespace

extern "C" size_t v3d_mesh_workspace_bytes(int nx, int ny, int nz) {
  if (!volume_ok(nx, ny, nz)) return 0;
  return mc_layout((long long)nx * ny * nz).total;
}

extern "C" int v3d_mesh_count_f32(const float* tsdf, int nx, int ny, int nz, int mode, int32_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(tsdf && counts && workspace, V3D_ERR_BAD_ARG, "v3d_mesh_count_f32: null argument");
  V3D_REQUIRE(mode == V3D_MESH_MODE_MESH || mode == V3D_MESH_MODE_POINT_CLOUD, V3D_ERR_BAD_ARG, "v3d_mesh_count_f32: mode=%d", mode);
  V3D_REQUIRE(volume_ok(nx, ny, nz), V3D_ERR_BAD_SHAPE, "v3d_mesh_count_f32: volume %d x %d x %d (positive, fewer than 2^31 voxels)",
              nx, ny, nz);
  const int n_vox = nx * ny * nz;
  const McLayout l = mc_layout(n_vox);
  V3D_REQUIRE(workspace_bytes >= l.total, V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_mesh_count_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  McMeta* meta = (McMeta*)base;
  unsigned long long* part_n = (unsigned long long*)(base + l.part_n);
  float* part_f = (float*)(base + l.part_f);
  unsigned char* mask = (unsigned char*)(base + l.mask);
  unsigned char* tcnt = (unsigned char*)(base + l.tcnt);
  unsigned* vofs = (unsigned*)(base + l.vofs);
  unsigned* tofs = (unsigned*)(base + l.tofs);
  const Dims d = {nx, ny, nz, n_vox};
  const unsigned grid = (unsigned)(((long long)n_vox + kTile - 1) / kTile);
  const bool mesh = mode == V3D_MESH_MODE_MESH;
  v3d::TimedScope ts("mesh_count", s);
  if (mesh)
    mc_classify_kernel<true><<<grid, kTile, 0, s>>>(tsdf, d, mask);
  else
    mc_classify_kernel<false><<<grid, kTile, 0, s>>>(tsdf, d, mask);
  V3D_CHECK_LAUNCH("mc_classify_kernel");
  if (mesh) {
    mc_tricount_kernel<<<grid, kTile, 0, s>>>(mask, d, tcnt);
    V3D_CHECK_LAUNCH("mc_tricount_kernel");
  }
  const int nb = (int)(grid < (unsigned)kRedBlocks ? grid : (unsigned)kRedBlocks);
  mc_totals_partial_kernel<<<nb, 256, 0, s>>>(tsdf, mask, mesh ? tcnt : nullptr, n_vox, part_n, part_f);
  V3D_CHECK_LAUNCH("mc_totals_partial_kernel");
  mc_totals_finish_kernel<<<1, 256, 0, s>>>(part_n, part_f, nb, mesh ? 1 : 0, meta, counts);
  V3D_CHECK_LAUNCH("mc_totals_finish_kernel");
  size_t tb = l.temp_bytes;
  V3D_CHECK_HIP(rocprim::exclusive_scan(base + l.temp, tb, rocprim::make_transform_iterator((const unsigned char*)mask, KeptCount()),
                                        vofs, 0u, (size_t)n_vox, rocprim::plus<unsigned>(), s));
  if (mesh) {
    tb = l.temp_bytes;
    V3D_CHECK_HIP(rocprim::exclusive_scan(base + l.temp, tb, rocprim::make_transform_iterator((const unsigned char*)tcnt, ByteCount()),
                                          tofs, 0u, (size_t)n_vox, rocprim::plus<unsigned>(), s));
  }
  return V3D_OK;
}

extern "C" int v3d_mesh_extract_f32(const float* tsdf, const float* color, int nx, int ny, int nz, double voxel_size,
                                    const float* origin_host, int mode, float* verts, uint8_t* colors, int v_cap, int32_t* tris,
                                    int f_cap, const void* workspace, size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(tsdf && origin_host && workspace, V3D_ERR_BAD_ARG, "v3d_mesh_extract_f32: null argument");
  V3D_REQUIRE(mode == V3D_MESH_MODE_MESH || mode == V3D_MESH_MODE_POINT_CLOUD, V3D_ERR_BAD_ARG, "v3d_mesh_extract_f32: mode=%d", mode);
  V3D_REQUIRE((color == nullptr) == (colors == nullptr) || v_cap == 0, V3D_ERR_BAD_ARG,
              "v3d_mesh_extract_f32: the colour volume and the colour output go together");
  V3D_REQUIRE(std::isfinite(voxel_size) && voxel_size > 0.0 && std::isfinite((float)voxel_size) && (float)voxel_size > 0.f,
              V3D_ERR_BAD_ARG, "v3d_mesh_extract_f32: voxel_size=%g (positive and finite)", voxel_size);
  V3D_REQUIRE(std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]), V3D_ERR_BAD_ARG,
              "v3d_mesh_extract_f32: origin is not finite");
  V3D_REQUIRE(volume_ok(nx, ny, nz), V3D_ERR_BAD_SHAPE, "v3d_mesh_extract_f32: volume %d x %d x %d (positive, fewer than 2^31 voxels)",
              nx, ny, nz);
  V3D_REQUIRE(v_cap >= 0 && f_cap >= 0, V3D_ERR_BAD_SHAPE, "v3d_mesh_extract_f32: v_cap=%d f_cap=%d", v_cap, f_cap);
  V3D_REQUIRE((v_cap == 0 || verts) && (f_cap == 0 || tris), V3D_ERR_BAD_ARG, "v3d_mesh_extract_f32: null argument");
  const int n_vox = nx * ny * nz;
  const McLayout l = mc_layout(n_vox);
  V3D_REQUIRE(workspace_bytes >= l.total, V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_mesh_extract_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const char* base = (const char*)workspace;
  const McMeta* meta = (const McMeta*)base;
  const unsigned char* mask = (const unsigned char*)(base + l.mask);
  const unsigned char* tcnt = (const unsigned char*)(base + l.tcnt);
  const unsigned* vofs = (const unsigned*)(base + l.vofs);
  const unsigned* tofs = (const unsigned*)(base + l.tofs);
  const Dims d = {nx, ny, nz, n_vox};
  const unsigned grid = (unsigned)(((long long)n_vox + kTile - 1) / kTile);
  const bool mesh = mode == V3D_MESH_MODE_MESH;
  const float vs = (float)voxel_size;
  v3d::TimedScope ts("mesh_extract", s);
  if (v_cap > 0) {
    if (mesh)
      mc_emit_vertices_kernel<true><<<grid, kTile, 0, s>>>(tsdf, color, d, vs, origin_host[0], origin_host[1], origin_host[2], mask, vofs,
                                                           meta, verts, colors, v_cap);
    else
      mc_emit_vertices_kernel<false><<<grid, kTile, 0, s>>>(tsdf, color, d, vs, origin_host[0], origin_host[1], origin_host[2], mask, vofs,
                                                            meta, verts, colors, v_cap);
    V3D_CHECK_LAUNCH("mc_emit_vertices_kernel");
  }
  if (mesh && f_cap > 0) {
    mc_emit_triangles_kernel<<<grid, kTile, 0, s>>>(d, mask, tcnt, vofs, tofs, meta, tris, f_cap);
    V3D_CHECK_LAUNCH("mc_emit_triangles_kernel");
  }
  return V3D_OK;
}
