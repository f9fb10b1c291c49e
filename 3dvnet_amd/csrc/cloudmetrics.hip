// Scoring of a fused point cloud (mv3d/eval/processresults.py:283-295, mv3d/eval/metricfunctions.py:70-124), on the device:
//
//   cloud down-sample    Open3D's documented VoxelDownSample, restated (parity-unpinned: the package is not available).
//                        Double-precision bounds and cell indices, 3 x 21-bit key x 2^42 + y 2^21 + z, stable rocPRIM radix sort
//                        of (key, row), heads by comparing neighbours, rocPRIM exclusive scan, then ONE thread per cell walks its
//                        rows in original order, sums in double, divides by the count and rounds once to fp32.  Output order:
//                        ascending key.  No atomics; the row count may come from a device word.
//   exact nearest neighbour   target rows sorted by the 30-bit Morton code of a fine cell (1024 per axis, edge a power of two);
//                        a coarser cell is a contiguous range of the sorted array, found through a table of the 64^3 level-4
//                        cells (and, below that level, a binary search inside one table range).  Queries are sorted by the same
//                        code, one thread per query.  At level L the 27 cells around the query are scanned, cells (and, inside
//                        coarse cells, level-4 / level-6 blocks) whose box is farther than the current best are skipped; the
//                        search ends when best < cell edge of level L, else it goes one level up; level 10 is the whole cloud.
//                        Exact and order-independent: the winner is the minimum of (fp32 distance, original row).
//   metric reduction     two distance arrays + threshold -> acc, comp, prec, recal, fscore in double; fixed two-stage sum.
//
// Why "best < edge" ends the search exactly: cell coordinates are floor((double(p) - origin) / edge) with a power-of-two edge,
// so a target row outside the 27 cells is more than one edge away from the query along some axis; fp32 subtraction, product,
// sum and square root are monotone, so its fp32 distance is >= the edge (a power of two, exact in fp32) > best.  The query's
// cell is clamped into the grid, which keeps that argument for queries outside the target's box.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::mul_rn;
using v3d::sub_rn;

constexpr int kRedBlocks = 256;
constexpr int kAxisBits = 10;                       // fine cells per axis = 1024; levels 0 .. 10
constexpr int kGrid = 1 << kAxisBits;
constexpr int kTabLevel = 4;                        // table of cell starts at level 4: 64 cells per axis
constexpr int kTabCells = 1 << (3 * (kAxisBits - kTabLevel));
constexpr double kMaxIndex = 2097152.0;             // 2^21 cells per axis of the down-sample key

struct DsMeta {           // device-resident status of a down-sample call (v3d_cloud_status)
  double vmin[3];
  double voxel;
  int count;              // input rows in use
  int error;              // 1 non-finite coordinate | 2 extent / voxel_size >= 2^21 | 4 voxel_size <= 0
  int n_out;
};

struct NnMeta {
  double org[3];
  double e0;              // fine cell edge, a power of two
};

// ---- bounds ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int rows_in_use(int n, const int* n_dev) {
  if (!n_dev) return n;
  const int c = *n_dev;
  return c < 0 ? 0 : (c > n ? n : c);
}

// per-block minima / maxima of the first rows_in_use rows and a non-finite flag: part[b * 7 + 0..2] min, 3..5 max, 6 flag
__global__ __launch_bounds__(256) void cloud_bounds_partial_kernel(const float* __restrict__ pts, int n, const int* __restrict__ n_dev,
                                                                    float* __restrict__ part) {
  const int cnt = rows_in_use(n, n_dev);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  float bad = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float v = pts[(size_t)i * 3 + d];
      lo[d] = fminf(lo[d], v);
      hi[d] = fmaxf(hi[d], v);
      if (!(fabsf(v) <= 3.4028234e38f)) bad = 1.f;
    }
  }
  __shared__ float s[7][256];
#pragma unroll
  for (int d = 0; d < 3; ++d) { s[d][threadIdx.x] = lo[d]; s[3 + d][threadIdx.x] = hi[d]; }
  s[6][threadIdx.x] = bad;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        s[d][threadIdx.x] = fminf(s[d][threadIdx.x], s[d][threadIdx.x + o]);
        s[3 + d][threadIdx.x] = fmaxf(s[3 + d][threadIdx.x], s[3 + d][threadIdx.x + o]);
      }
      s[6][threadIdx.x] = fmaxf(s[6][threadIdx.x], s[6][threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x < 7) part[blockIdx.x * 7 + threadIdx.x] = s[threadIdx.x][0];
}

// one wave: the partials over the 64 lanes, then shuffles (minima / maxima do not depend on the order)
__device__ __forceinline__ void bounds_finish(const float* __restrict__ part, int nblocks, float lo[3], float hi[3], float& bad) {
  for (int d = 0; d < 3; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
  bad = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += 64) {
    for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], part[b * 7 + d]); hi[d] = fmaxf(hi[d], part[b * 7 + 3 + d]); }
    bad = fmaxf(bad, part[b * 7 + 6]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], __shfl_xor(lo[d], o)); hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o)); }
    bad = fmaxf(bad, __shfl_xor(bad, o));
  }
}

// ---- voxel down-sample -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void ds_finish_kernel(const float* __restrict__ part, int nblocks, int n, const int* __restrict__ n_dev,
                                                        double voxel, DsMeta* __restrict__ meta, int* __restrict__ out_count) {
  float lo[3], hi[3], bad;
  bounds_finish(part, nblocks, lo, hi, bad);
  if (threadIdx.x != 0) return;
  const int cnt = rows_in_use(n, n_dev);
  int err = 0;
  if (!(voxel > 0.0) || !(voxel <= 1.7e308)) err |= 4;
  if (cnt > 0 && bad != 0.f) err |= 1;
  for (int d = 0; d < 3; ++d) {
    const double vmin = (double)lo[d] - 0.5 * voxel;          // Open3D: min_bound - voxel_size / 2
    meta->vmin[d] = vmin;
    if (cnt > 0 && !err && !(floor(((double)hi[d] - vmin) / voxel) < kMaxIndex)) err |= 2;
  }
  meta->voxel = voxel;
  meta->count = cnt;
  meta->error = err;
  meta->n_out = 0;
  if (err) *out_count = -err;          // a negative count word = the error bits (v3d_cloud_status has the text)
  else if (cnt == 0) *out_count = 0;
}

__global__ __launch_bounds__(256) void ds_keys_kernel(const float* __restrict__ pts, int n, const DsMeta* __restrict__ meta,
                                                       unsigned long long* __restrict__ keys, unsigned* __restrict__ rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned long long key = ~0ull;                              // rows not in use sort behind every cell
  if (i < meta->count && !meta->error) {
    key = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      double c = floor(((double)pts[(size_t)i * 3 + d] - meta->vmin[d]) / meta->voxel);
      c = fmin(fmax(c, 0.0), kMaxIndex - 1.0);                 // in range already (checked in ds_finish_kernel)
      key = (key << 21) | (unsigned long long)c;
    }
  }
  keys[i] = key;
  rows[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void ds_heads_kernel(const unsigned long long* __restrict__ keys, int n, const DsMeta* __restrict__ meta,
                                                        unsigned* __restrict__ head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  head[i] = (i < meta->count && !meta->error && (i == 0 || keys[i] != keys[i - 1])) ? 1u : 0u;
}

// one thread per cell: the thread on the cell's first sorted row walks the cell.  The sort is stable, so the walk visits the
// member rows in original order.
__global__ __launch_bounds__(256) void ds_reduce_kernel(const float* __restrict__ pts, const float* __restrict__ attr, int n_attr,
                                                         const unsigned long long* __restrict__ keys, const unsigned* __restrict__ rows,
                                                         const unsigned* __restrict__ head, const unsigned* __restrict__ seg_of,
                                                         DsMeta* __restrict__ meta, float* __restrict__ out_pts,
                                                         float* __restrict__ out_attr, int* __restrict__ out_count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int cnt = meta->count;
  if (i >= cnt || meta->error || !head[i]) return;
  const unsigned long long key = keys[i];
  const size_t seg = seg_of[i];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  int j = i;
  for (; j < cnt && keys[j] == key; ++j) {
    const float* p = pts + (size_t)rows[j] * 3;
    sx += (double)p[0]; sy += (double)p[1]; sz += (double)p[2];
  }
  const double m = (double)(j - i);
  out_pts[seg * 3 + 0] = (float)(sx / m);
  out_pts[seg * 3 + 1] = (float)(sy / m);
  out_pts[seg * 3 + 2] = (float)(sz / m);
  for (int a = 0; a < n_attr; ++a) {
    double s = 0.0;
    for (int k = i; k < j; ++k) s += (double)attr[(size_t)rows[k] * n_attr + a];
    out_attr[seg * n_attr + a] = (float)(s / m);
  }
  if (j == cnt) {                       // the last cell knows the number of cells
    *out_count = (int)seg + 1;
    meta->n_out = (int)seg + 1;
  }
}

struct DsLayout { size_t part, keys_in, keys_out, rows_in, rows_out, head, seg, temp, temp_bytes, total; };

DsLayout ds_layout(int n) {
  DsLayout l;
  const size_t m = n > 0 ? (size_t)n : 1;
  size_t b1 = 0, b2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b1, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                  (unsigned*)nullptr, m, 0, 64, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, b2, (unsigned*)nullptr, (unsigned*)nullptr, 0u, m, rocprim::plus<unsigned>(), (hipStream_t)0);
  l.temp_bytes = v3d::align_up(b1 > b2 ? b1 : b2, 256);
  size_t o = 256;
  l.part = o; o += v3d::align_up(kRedBlocks * 7 * sizeof(float), 256);
  l.keys_in = o; o += v3d::align_up(m * 8, 256);
  l.keys_out = o; o += v3d::align_up(m * 8, 256);
  l.rows_in = o; o += v3d::align_up(m * 4, 256);
  l.rows_out = o; o += v3d::align_up(m * 4, 256);
  l.head = o; o += v3d::align_up(m * 4, 256);
  l.seg = o; o += v3d::align_up(m * 4, 256);
  l.temp = o; o += l.temp_bytes;
  l.total = o;
  return l;
}

// ---- nearest neighbour -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned spread10(unsigned x) {     // bits 0..9 -> every third bit
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}
__device__ __forceinline__ unsigned compact10(unsigned x) {
  x &= 0x09249249u;
  x = (x ^ (x >> 2)) & 0x030c30c3u;
  x = (x ^ (x >> 4)) & 0x0300f00fu;
  x = (x ^ (x >> 8)) & 0x030000ffu;
  x = (x ^ (x >> 16)) & 0x3ffu;
  return x;
}
__device__ __forceinline__ unsigned morton3(int x, int y, int z) { return spread10(x) | (spread10(y) << 1) | (spread10(z) << 2); }

// fine cell of a coordinate, clamped into the grid (NaN -> 0)
__device__ __forceinline__ int fine_cell(double t, double e0) { return (int)fmin(fmax(floor(t / e0), 0.0), (double)(kGrid - 1)); }

__global__ __launch_bounds__(64) void nn_finish_kernel(const float* __restrict__ part, int nblocks, NnMeta* __restrict__ meta) {
  float lo[3], hi[3], bad;
  bounds_finish(part, nblocks, lo, hi, bad);
  if (threadIdx.x != 0) return;
  double ext = 0.0;
  for (int d = 0; d < 3; ++d) {
    const bool ok = fabsf(lo[d]) <= 3.4028234e38f && fabsf(hi[d]) <= 3.4028234e38f;
    meta->org[d] = ok ? (double)lo[d] : 0.0;
    if (ok) ext = fmax(ext, (double)hi[d] - (double)lo[d]);
  }
  int k = -40;                                                  // smallest power of two with extent / edge < 1023
  while (k < 140 && !(ext < 1023.0 * ldexp(1.0, k))) ++k;
  meta->e0 = ldexp(1.0, k);
}

__global__ __launch_bounds__(256) void nn_codes_kernel(const float* __restrict__ pts, int n, const NnMeta* __restrict__ meta,
                                                        unsigned* __restrict__ codes, unsigned* __restrict__ rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double e0 = meta->e0;
  const int gx = fine_cell((double)pts[(size_t)i * 3 + 0] - meta->org[0], e0);
  const int gy = fine_cell((double)pts[(size_t)i * 3 + 1] - meta->org[1], e0);
  const int gz = fine_cell((double)pts[(size_t)i * 3 + 2] - meta->org[2], e0);
  codes[i] = morton3(gx, gy, gz);
  rows[i] = (unsigned)i;
}

// sorted target rows as 16-byte records (x, y, z, original row)
__global__ __launch_bounds__(256) void nn_gather_kernel(const float* __restrict__ pts, const unsigned* __restrict__ rows, int n,
                                                         float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned r = rows[i];
  out[i] = make_float4(pts[(size_t)r * 3], pts[(size_t)r * 3 + 1], pts[(size_t)r * 3 + 2], __int_as_float((int)r));
}

__device__ __forceinline__ int lower_bound_u32(const unsigned* __restrict__ a, int lo, int hi, unsigned key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// tab[t] = first sorted row whose code is >= t << 12 (t = Morton code of a level-4 cell), tab[kTabCells] = n
__global__ __launch_bounds__(256) void nn_table_kernel(const unsigned* __restrict__ codes, int n, int* __restrict__ tab) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t > kTabCells) return;
  tab[t] = t == kTabCells ? n : lower_bound_u32(codes, 0, n, (unsigned)t << (3 * kTabLevel));
}

// lower bound of the fp32 distance along one axis from the query (grid-relative coordinate t) to cell c of edge e: computed in
// double, rounded to fp32 and moved down by more than the roundings can have moved it up
__device__ __forceinline__ float axis_gap(double t, int c, double e, float slack) {
  const double lo = (double)c * e;
  const double g = fmax(fmax(lo - t, t - (lo + e)), 0.0);
  return fmaxf((float)g * 0.999999f - slack, 0.f);
}
__device__ __forceinline__ float box_bound(double tx, double ty, double tz, int cx, int cy, int cz, double e, float slack) {
  const float gx = axis_gap(tx, cx, e, slack), gy = axis_gap(ty, cy, e, slack), gz = axis_gap(tz, cz, e, slack);
  return add_rn(add_rn(mul_rn(gx, gx), mul_rn(gy, gy)), mul_rn(gz, gz));       // the same monotone chain as a point's
}

// rows [a, b) of the sorted target against the query.  best_hi is an upper bound on the squared sums whose root can still be
// <= best_d, so the square root and the exact (distance, row) comparison run only for candidates
__device__ __forceinline__ void scan_rows(const float4* __restrict__ tp, int a, int b, float qx, float qy, float qz, float& best_d,
                                          float& best_hi, int& best_i) {
  for (int j = a; j < b; ++j) {
    const float4 p = tp[j];
    const float dx = sub_rn(p.x, qx), dy = sub_rn(p.y, qy), dz = sub_rn(p.z, qz);
    const float s = add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz));
    if (s <= best_hi) {
      const float d = sqrtf(s);
      const int r = __float_as_int(p.w);
      if (d < best_d || (d == best_d && r < best_i)) {
        best_d = d;
        best_i = r;
        best_hi = add_rn(mul_rn(mul_rn(d, d), 1.0000005f), 1e-37f);
      }
    }
  }
}

__global__ __launch_bounds__(256) void nn_query_kernel(const float* __restrict__ query, const unsigned* __restrict__ qrows, int n_query,
                                                        const float4* __restrict__ tp, const unsigned* __restrict__ tcodes,
                                                        const int* __restrict__ tab, const NnMeta* __restrict__ meta,
                                                        int* __restrict__ out_idx, float* __restrict__ out_dist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_query) return;
  const unsigned row = qrows[i];
  const float qx = query[(size_t)row * 3], qy = query[(size_t)row * 3 + 1], qz = query[(size_t)row * 3 + 2];
  const double e0 = meta->e0;
  const double tx = (double)qx - meta->org[0], ty = (double)qy - meta->org[1], tz = (double)qz - meta->org[2];
  const int gx = fine_cell(tx, e0), gy = fine_cell(ty, e0), gz = fine_cell(tz, e0);
  const float slack = (float)(e0 * 1e-9);
  const double e_tab = ldexp(e0, kTabLevel), e_blk = ldexp(e0, kTabLevel + 2);

  float best_d = INFINITY, best_hi = INFINITY;
  int best_i = 0x7fffffff;
  for (int L = 0; L <= kAxisBits; ++L) {
    const double e = ldexp(e0, L);
    const int ncell = kGrid >> L;
    const int cx = gx >> L, cy = gy >> L, cz = gz >> L;
    for (int k = 0; k < 27; ++k) {
      const int k9 = k / 9, k3 = (k - k9 * 9) / 3;
      const int ix = cx + (k - k9 * 9 - k3 * 3) - 1, iy = cy + k3 - 1, iz = cz + k9 - 1;
      if ((unsigned)ix >= (unsigned)ncell || (unsigned)iy >= (unsigned)ncell || (unsigned)iz >= (unsigned)ncell) continue;
      if (box_bound(tx, ty, tz, ix, iy, iz, e, slack) > best_hi) continue;
      const unsigned prefix = morton3(ix, iy, iz);
      if (L <= kTabLevel) {
        const unsigned t = prefix >> (3 * (kTabLevel - L));
        int a = tab[t], b = tab[t + 1];
        if (L < kTabLevel && a < b) {
          const unsigned first = prefix << (3 * L);
          a = lower_bound_u32(tcodes, a, b, first);
          b = lower_bound_u32(tcodes, a, b, first + (1u << (3 * L)));
        }
        scan_rows(tp, a, b, qx, qy, qz, best_d, best_hi, best_i);
      } else {
        // a coarse cell = a run of level-4 cells in the table; blocks of 64 (level 6) and single cells are skipped when empty or
        // farther than the best
        const int sh = 3 * (L - kTabLevel);
        const unsigned t0 = prefix << sh, t1 = (prefix + 1u) << sh;
        if (tab[t0] == tab[t1]) continue;
        for (unsigned t = t0; t < t1; ++t) {
          if ((t & 63u) == 0u && t + 64u <= t1) {
            const unsigned c = t >> 6;
            if (tab[t] == tab[t + 64] ||
                box_bound(tx, ty, tz, (int)compact10(c), (int)compact10(c >> 1), (int)compact10(c >> 2), e_blk, slack) > best_hi) {
              t += 63u;
              continue;
            }
          }
          const int a = tab[t], b = tab[t + 1];
          if (a == b) continue;
          if (box_bound(tx, ty, tz, (int)compact10(t), (int)compact10(t >> 1), (int)compact10(t >> 2), e_tab, slack) > best_hi) continue;
          scan_rows(tp, a, b, qx, qy, qz, best_d, best_hi, best_i);
        }
      }
    }
    if ((double)best_d < e) break;
  }
  out_idx[row] = best_i == 0x7fffffff ? -1 : best_i;
  out_dist[row] = best_d;
}

__global__ __launch_bounds__(256) void nn_fill_kernel(int* __restrict__ idx, float* __restrict__ dist, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  idx[i] = -1;
  dist[i] = INFINITY;
}

struct NnLayout { size_t part, tcode_in, tcode, trow_in, trow, tpts, tab, qcode_in, qcode, qrow_in, qrow, temp, temp_bytes, total; };

NnLayout nn_layout(int n_target, int n_query) {
  NnLayout l;
  const size_t nt = n_target > 0 ? (size_t)n_target : 1, nq = n_query > 0 ? (size_t)n_query : 1;
  size_t b1 = 0, b2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b1, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, nt, 0,
                                  3 * kAxisBits, (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, b2, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, nq, 0,
                                  3 * kAxisBits, (hipStream_t)0);
  l.temp_bytes = v3d::align_up(b1 > b2 ? b1 : b2, 256);
  size_t o = 256;
  l.part = o; o += v3d::align_up(kRedBlocks * 7 * sizeof(float), 256);
  l.tcode_in = o; o += v3d::align_up(nt * 4, 256);
  l.tcode = o; o += v3d::align_up(nt * 4, 256);
  l.trow_in = o; o += v3d::align_up(nt * 4, 256);
  l.trow = o; o += v3d::align_up(nt * 4, 256);
  l.tpts = o; o += v3d::align_up(nt * 16, 256);
  l.tab = o; o += v3d::align_up(((size_t)kTabCells + 1) * 4, 256);
  l.qcode_in = o; o += v3d::align_up(nq * 4, 256);
  l.qcode = o; o += v3d::align_up(nq * 4, 256);
  l.qrow_in = o; o += v3d::align_up(nq * 4, 256);
  l.qrow = o; o += v3d::align_up(nq * 4, 256);
  l.temp = o; o += l.temp_bytes;
  l.total = o;
  return l;
}

// ---- metrics -----------------------------------------------------------------------------------------------------------------

// stage 1: block b of array a (blockIdx.y) sums its grid-stride share in double and counts double(d) < threshold; the tree in
// LDS has a fixed shape, so the partials do not depend on timing
__global__ __launch_bounds__(256) void metrics_partial_kernel(const float* __restrict__ d1, int n1, const float* __restrict__ d2, int n2,
                                                               double threshold, double* __restrict__ part) {
  const float* __restrict__ d = blockIdx.y ? d2 : d1;
  const int n = blockIdx.y ? n2 : n1;
  double sum = 0.0, hit = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += kRedBlocks * 256) {
    const double v = (double)d[i];
    sum += v;
    hit += v < threshold ? 1.0 : 0.0;
  }
  __shared__ double s[2][256];
  s[0][threadIdx.x] = sum;
  s[1][threadIdx.x] = hit;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      s[0][threadIdx.x] += s[0][threadIdx.x + o];
      s[1][threadIdx.x] += s[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) part[((size_t)blockIdx.y * kRedBlocks + blockIdx.x) * 2 + threadIdx.x] = s[threadIdx.x][0];
}

// stage 2: one workgroup, the same fixed tree over the 256 partials of each array -> acc, comp, prec, recal, fscore
__global__ __launch_bounds__(256) void metrics_finish_kernel(const double* __restrict__ part, int n1, int n2, double* __restrict__ out) {
  __shared__ double s[4][256];
  for (int k = 0; k < 4; ++k) s[k][threadIdx.x] = part[((size_t)(k >> 1) * kRedBlocks + threadIdx.x) * 2 + (k & 1)];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int k = 0; k < 4; ++k) s[k][threadIdx.x] += s[k][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double acc = s[0][0] / (double)n1, prec = s[1][0] / (double)n1;       // an empty array gives 0 / 0 = NaN, as np.mean does
  const double comp = s[2][0] / (double)n2, recal = s[3][0] / (double)n2;
  out[0] = acc;
  out[1] = comp;
  out[2] = prec;
  out[3] = recal;
  out[4] = 2.0 * prec * recal / (prec + recal + 1e-8);
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------------

extern "C" size_t v3d_cloud_downsample_workspace_bytes(int n) {
  if (n < 0) return 0;
  return ds_layout(n).total;
}

extern "C" int v3d_cloud_downsample_f32(const float* pts, const float* attr, int n_attr, int n, const int32_t* n_dev, double voxel_size,
                                        float* out_pts, float* out_attr, int32_t* out_count, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  V3D_REQUIRE(out_count && workspace, V3D_ERR_BAD_ARG, "v3d_cloud_downsample_f32: null argument");
  V3D_REQUIRE(n >= 0, V3D_ERR_BAD_SHAPE, "v3d_cloud_downsample_f32: n=%d", n);
  V3D_REQUIRE(n == 0 || (pts && out_pts), V3D_ERR_BAD_ARG, "v3d_cloud_downsample_f32: null argument");
  V3D_REQUIRE(n_attr >= 0 && n_attr <= 64, V3D_ERR_BAD_SHAPE, "v3d_cloud_downsample_f32: n_attr=%d (0..64)", n_attr);
  V3D_REQUIRE(n_attr == 0 || n == 0 || (attr && out_attr), V3D_ERR_BAD_ARG,
              "v3d_cloud_downsample_f32: n_attr=%d needs attr and out_attr", n_attr);
  V3D_REQUIRE((long long)n * (n_attr > 3 ? n_attr : 3) < (1ll << 40), V3D_ERR_BAD_SHAPE, "v3d_cloud_downsample_f32: too many rows");
  const DsLayout l = ds_layout(n);
  V3D_REQUIRE(workspace_bytes >= l.total, V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_cloud_downsample_f32: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)workspace;
  DsMeta* meta = (DsMeta*)base;
  float* part = (float*)(base + l.part);
  unsigned long long* keys_in = (unsigned long long*)(base + l.keys_in);
  unsigned long long* keys = (unsigned long long*)(base + l.keys_out);
  unsigned* rows_in = (unsigned*)(base + l.rows_in);
  unsigned* rows = (unsigned*)(base + l.rows_out);
  unsigned* head = (unsigned*)(base + l.head);
  unsigned* seg = (unsigned*)(base + l.seg);
  size_t tb = l.temp_bytes;
  const int nb = n > 0 ? min(kRedBlocks, (n + 255) / 256) : 1;
  v3d::TimedScope ts("cloud_downsample", s);
  cloud_bounds_partial_kernel<<<nb, 256, 0, s>>>(pts, n, n_dev, part);
  V3D_CHECK_LAUNCH("cloud_bounds_partial_kernel");
  ds_finish_kernel<<<1, 64, 0, s>>>(part, nb, n, n_dev, voxel_size, meta, out_count);
  V3D_CHECK_LAUNCH("ds_finish_kernel");
  if (n == 0) return V3D_OK;
  const int grid = (n + 255) / 256;
  ds_keys_kernel<<<grid, 256, 0, s>>>(pts, n, meta, keys_in, rows_in);
  V3D_CHECK_LAUNCH("ds_keys_kernel");
  V3D_CHECK_HIP(rocprim::radix_sort_pairs(base + l.temp, tb, keys_in, keys, rows_in, rows, (size_t)n, 0, 64, s));
  ds_heads_kernel<<<grid, 256, 0, s>>>(keys, n, meta, head);
  V3D_CHECK_LAUNCH("ds_heads_kernel");
  tb = l.temp_bytes;
  V3D_CHECK_HIP(rocprim::exclusive_scan(base + l.temp, tb, head, seg, 0u, (size_t)n, rocprim::plus<unsigned>(), s));
  ds_reduce_kernel<<<grid, 256, 0, s>>>(pts, attr, n_attr, keys, rows, head, seg, meta, out_pts, out_attr, out_count);
  V3D_CHECK_LAUNCH("ds_reduce_kernel");
  return V3D_OK;
}

extern "C" int v3d_cloud_status(const void* workspace, size_t workspace_bytes, int32_t* n_out_host, void* stream) {
  V3D_REQUIRE(workspace && workspace_bytes >= 256, V3D_ERR_BAD_ARG, "v3d_cloud_status: not a down-sample workspace");
  DsMeta m;
  V3D_CHECK_HIP(hipMemcpyAsync(&m, workspace, sizeof(DsMeta), hipMemcpyDeviceToHost, (hipStream_t)stream));
  V3D_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (n_out_host) *n_out_host = m.error ? 0 : m.n_out;
  V3D_REQUIRE((m.error & 4) == 0, V3D_ERR_BAD_ARG, "cloud down-sample: voxel_size=%g must be positive and finite", m.voxel);
  V3D_REQUIRE((m.error & 1) == 0, V3D_ERR_BAD_ARG, "cloud down-sample: the cloud holds a non-finite coordinate");
  V3D_REQUIRE((m.error & 2) == 0, V3D_ERR_BAD_SHAPE, "cloud down-sample: extent / voxel_size (%g) reaches 2^21 cells on an axis", m.voxel);
  return V3D_OK;
}

extern "C" size_t v3d_nn_workspace_bytes(int n_target, int n_query) {
  if (n_target < 0 || n_query < 0) return 0;
  return nn_layout(n_target, n_query).total;
}

extern "C" int v3d_nn_query_f32(const float* target, int n_target, const float* query, int n_query, int32_t* idx, float* dist,
                                void* workspace, size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(n_target >= 0 && n_query >= 0, V3D_ERR_BAD_SHAPE, "v3d_nn_query_f32: n_target=%d n_query=%d", n_target, n_query);
  V3D_REQUIRE(n_target < (1 << 30) && n_query < (1 << 30), V3D_ERR_BAD_SHAPE, "v3d_nn_query_f32: more than 2^30 rows");
  if (n_query == 0) return V3D_OK;
  V3D_REQUIRE(query && idx && dist, V3D_ERR_BAD_ARG, "v3d_nn_query_f32: null argument");
  hipStream_t s = (hipStream_t)stream;
  const int qgrid = (n_query + 255) / 256;
  if (n_target == 0) {                     // no neighbour: index -1 at distance +inf
    nn_fill_kernel<<<qgrid, 256, 0, s>>>(idx, dist, n_query);
    V3D_CHECK_LAUNCH("nn_fill_kernel");
    return V3D_OK;
  }
  V3D_REQUIRE(target && workspace, V3D_ERR_BAD_ARG, "v3d_nn_query_f32: null argument");
  const NnLayout l = nn_layout(n_target, n_query);
  V3D_REQUIRE(workspace_bytes >= l.total, V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_nn_query_f32: workspace too small");
  char* base = (char*)workspace;
  NnMeta* meta = (NnMeta*)base;
  float* part = (float*)(base + l.part);
  unsigned* tcode_in = (unsigned*)(base + l.tcode_in);
  unsigned* tcode = (unsigned*)(base + l.tcode);
  unsigned* trow_in = (unsigned*)(base + l.trow_in);
  unsigned* trow = (unsigned*)(base + l.trow);
  float4* tpts = (float4*)(base + l.tpts);
  int* tab = (int*)(base + l.tab);
  unsigned* qcode_in = (unsigned*)(base + l.qcode_in);
  unsigned* qcode = (unsigned*)(base + l.qcode);
  unsigned* qrow_in = (unsigned*)(base + l.qrow_in);
  unsigned* qrow = (unsigned*)(base + l.qrow);
  const int tgrid = (n_target + 255) / 256;
  const int nb = min(kRedBlocks, tgrid);
  size_t tb = l.temp_bytes;
  {
    v3d::TimedScope ts("nn_build", s);
    cloud_bounds_partial_kernel<<<nb, 256, 0, s>>>(target, n_target, nullptr, part);
    V3D_CHECK_LAUNCH("cloud_bounds_partial_kernel");
    nn_finish_kernel<<<1, 64, 0, s>>>(part, nb, meta);
    V3D_CHECK_LAUNCH("nn_finish_kernel");
    nn_codes_kernel<<<tgrid, 256, 0, s>>>(target, n_target, meta, tcode_in, trow_in);
    V3D_CHECK_LAUNCH("nn_codes_kernel");
    V3D_CHECK_HIP(rocprim::radix_sort_pairs(base + l.temp, tb, tcode_in, tcode, trow_in, trow, (size_t)n_target, 0, 3 * kAxisBits, s));
    nn_gather_kernel<<<tgrid, 256, 0, s>>>(target, trow, n_target, tpts);
    V3D_CHECK_LAUNCH("nn_gather_kernel");
    nn_table_kernel<<<(kTabCells + 1 + 255) / 256, 256, 0, s>>>(tcode, n_target, tab);
    V3D_CHECK_LAUNCH("nn_table_kernel");
  }
  {
    v3d::TimedScope ts("nn_query", s);
    nn_codes_kernel<<<qgrid, 256, 0, s>>>(query, n_query, meta, qcode_in, qrow_in);
    V3D_CHECK_LAUNCH("nn_codes_kernel");
    tb = l.temp_bytes;
    V3D_CHECK_HIP(rocprim::radix_sort_pairs(base + l.temp, tb, qcode_in, qcode, qrow_in, qrow, (size_t)n_query, 0, 3 * kAxisBits, s));
    nn_query_kernel<<<qgrid, 256, 0, s>>>(query, qrow, n_query, tpts, tcode, tab, meta, idx, dist);
    V3D_CHECK_LAUNCH("nn_query_kernel");
  }
  return V3D_OK;
}

extern "C" size_t v3d_cloud_metrics_workspace_bytes(void) { return (size_t)2 * kRedBlocks * 2 * sizeof(double); }

extern "C" int v3d_cloud_metrics_f64(const float* dist_pred, int n_pred, const float* dist_target, int n_target, double threshold,
                                     double* out, void* workspace, size_t workspace_bytes, void* stream) {
  V3D_REQUIRE(out && workspace, V3D_ERR_BAD_ARG, "v3d_cloud_metrics_f64: null argument");
  V3D_REQUIRE(n_pred >= 0 && n_target >= 0, V3D_ERR_BAD_SHAPE, "v3d_cloud_metrics_f64: n_pred=%d n_target=%d", n_pred, n_target);
  V3D_REQUIRE((n_pred == 0 || dist_pred) && (n_target == 0 || dist_target), V3D_ERR_BAD_ARG, "v3d_cloud_metrics_f64: null argument");
  V3D_REQUIRE(threshold > 0.0, V3D_ERR_BAD_ARG, "v3d_cloud_metrics_f64: threshold=%g must be positive", threshold);
  V3D_REQUIRE(workspace_bytes >= v3d_cloud_metrics_workspace_bytes(), V3D_ERR_WORKSPACE_TOO_SMALL,
              "v3d_cloud_metrics_f64: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  v3d::TimedScope ts("cloud_metrics", s);
  metrics_partial_kernel<<<dim3(kRedBlocks, 2), 256, 0, s>>>(dist_pred, n_pred, dist_target, n_target, threshold, (double*)workspace);
  V3D_CHECK_LAUNCH("metrics_partial_kernel");
  metrics_finish_kernel<<<1, 256, 0, s>>>((const double*)workspace, n_pred, n_target, out);
  V3D_CHECK_LAUNCH("metrics_finish_kernel");
  return V3D_OK;
}
