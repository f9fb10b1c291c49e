// Exact per-axis order statistics of a 3-D point set by radix selection on the fp32 bit patterns: what the volume bounds of a
// scene need (mv3d/eval/processresults.py:324-357 takes two quantiles per axis of the back-projected depths) without the
// points ever existing in memory.
//
//   order_stats_pass_kernel<P>    one counting pass over the input.  The monotone 32-bit key of a coordinate is cut into three
//                                 digits of 11 + 11 + 10 bits, most significant first.  Pass 0 counts the top digit of every
//                                 axis; pass 1 / 2 count the next digit of the keys whose higher digits equal the prefix of a
//                                 GROUP.  A group is a distinct (axis, prefix) among the (quantile, axis, lo / hi) targets:
//                                 targets that sit in the same bin share one histogram.
//   order_stats_narrow_kernel<P>  one workgroup between the passes: per target, the bin of its group's histogram that holds
//                                 its rank, and the rank that is left inside that bin; then the groups of the next pass.  After
//                                 pass 0 it also derives the count and the ranks (float64), after pass 2 it writes the values.
//
// The input is re-read by every pass: either a cloud [N, 3], or depth maps [n, h, w] with the inverse 4 x 4 projections
// [n, 16], back-projected in registers (include/v3d.h pins that arithmetic: every operation rounded on its own).  A row with a
// NaN coordinate counts on no axis.
//
// Histograms: a workgroup counts in LDS -- kSlots groups of 2048 uint32 bins = 48 KiB, so 3 workgroups of 512 threads (24 waves)
// per CU of the 160 KiB; more than kSlots groups (the lo / hi targets of an axis fell into different bins, or more than two
// quantiles) are served in further rounds of the same launch, each re-reading the input.  The non-zero bins are added to the
// global histogram with integer atomics: integer sums do not depend on the order, so repeated launches are bit-identical.
// Contention: the coordinates of real scenes share sign and exponent, so in pass 0 most lanes of a wave hit the same bin.  A
// wave therefore first counts the bin of its first pending lane once for every lane that shares it (ballot + one LDS add by
// that lane), twice over, and only what is left goes to per-lane LDS atomics.
#include <cmath>
#include <cstdint>

#include "v3d_common.h"

namespace {

using v3d::add_rn;
using v3d::mul_rn;

constexpr int kThreads = 512;                 // per workgroup of a counting pass
constexpr int kPerThread = 4;                 // points per thread and tile
constexpr int kTile = kThreads * kPerThread;  // 2048 points
constexpr int kBins = 2048;                   // bins of the widest digit
constexpr int kSlots = 6;                     // group histograms a workgroup holds in LDS at once
constexpr int kMaxQ = 4;
constexpr int kMaxTargets = kMaxQ * 3 * 2;
constexpr int kPeel = 2;                      // wave-aggregated adds before the per-lane atomics
constexpr size_t kHeaderBytes = 1024;

__host__ __device__ constexpr int digit_bits(int pass) { return pass == 2 ? 10 : 11; }
__host__ __device__ constexpr int digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }

// the state that travels from kernel to kernel, at the head of the workspace; the histograms follow at kHeaderBytes
struct Work {
  uint32_t count;                       // rows kept
  uint32_t n_groups;                    // groups of the coming pass (0: nothing left to count)
  uint32_t group_axis[kMaxTargets];
  uint32_t group_prefix[kMaxTargets];   // the digits decided so far
  uint32_t target_group[kMaxTargets];
  uint32_t target_rank[kMaxTargets];    // rank among the keys of the target's group
};
static_assert(sizeof(Work) <= kHeaderBytes, "Work must fit the header");

struct Quantiles {
  double q[kMaxQ];
  int n_q;
};

struct Source {
  const float* data;       // cloud [n_pts, 3], or depths [n, h, w]
  const float* proj_inv;   // [n, 16], row major (fused entry point)
  unsigned n_pts;          // rows / pixels
  unsigned hw, w;
};

__device__ __forceinline__ float div_rn(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

// monotone over all non-NaN floats: -inf lowest, +inf highest
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ uint32_t bits_of_key(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// row r of Pi . [x, y, 1, 1 / d], left to right
__device__ __forceinline__ float row_dot(const float* __restrict__ P, float x, float y, float inv) {
  return add_rn(add_rn(add_rn(mul_rn(P[0], x), mul_rn(P[1], y)), P[2]), mul_rn(P[3], inv));
}

// One point per lane -> its three keys; false when the lane has no point or the row holds a NaN.  Called by whole waves.
template <bool FUSED>
__device__ __forceinline__ bool load_keys(const Source& S, unsigned i, float first, uint32_t key[3]) {
  const bool in = i < S.n_pts;
  float p[3] = {0.f, 0.f, 0.f};
  if (FUSED) {
    unsigned view = 0;
    float x = 0.f, y = 0.f;
    if (in) {
      view = i / S.hw;
      const unsigned rem = i - view * S.hw, iy = rem / S.w;
      x = (float)(rem - iy * S.w);
      y = (float)iy;
    }
    // the lanes of a wave nearly always share a view: its matrix is read once per wave, through a uniform address
    bool todo = in;
    while (__ballot(todo)) {
      if (todo) {
        const unsigned v0 = (unsigned)__builtin_amdgcn_readfirstlane((int)view);
        if (view == v0) {
          const float* __restrict__ P = S.proj_inv + (size_t)v0 * 16;
          const float inv = div_rn(1.f, first);
          const float X3 = row_dot(P + 12, x, y, inv);
#pragma unroll
          for (int a = 0; a < 3; ++a) p[a] = div_rn(row_dot(P + 4 * a, x, y, inv), X3);
          todo = false;
        }
      }
    }
  } else if (in) {
    p[0] = first;
    p[1] = S.data[(size_t)i * 3 + 1];
    p[2] = S.data[(size_t)i * 3 + 2];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) key[a] = key_of(p[a]);
  return in && !(p[0] != p[0] || p[1] != p[1] || p[2] != p[2]);
}

// ++hist[bin] for every lane with `on`; called by whole waves (see the head of the file)
__device__ __forceinline__ void hist_add(uint32_t* hist, uint32_t bin, bool on) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int r = 0; r < kPeel; ++r) {
    const unsigned long long pend = __ballot(on);
    if (!pend) return;
    const int leader = __ffsll((long long)pend) - 1;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
    const bool same = on && bin == b0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&hist[b0], (uint32_t)__popcll(m));
    on = on && !same;
  }
  if (on) atomicAdd(&hist[bin], 1u);
}

template <int PASS, bool FUSED>
__global__ __launch_bounds__(kThreads) void order_stats_pass_kernel(Source S, const Work* __restrict__ work, uint32_t* __restrict__ hist,
                                                                    int n_tiles) {
  constexpr int kB = 1 << digit_bits(PASS);
  constexpr int kLds = (PASS == 0 ? 3 : kSlots) * kB;
  __shared__ uint32_t lds[kLds];
  __shared__ uint32_t g_axis[kSlots], g_prefix[kSlots];
  const int n_groups = PASS == 0 ? 3 : (int)work->n_groups;       // uniform; at most kMaxTargets
  for (int g0 = 0; g0 < n_groups; g0 += kSlots) {
    const int n_here = min(PASS == 0 ? 3 : kSlots, n_groups - g0);
    for (int b = (int)threadIdx.x; b < kLds; b += kThreads) lds[b] = 0u;
    if (PASS != 0 && (int)threadIdx.x < n_here) {
      g_axis[threadIdx.x] = min(work->group_axis[g0 + threadIdx.x], 2u);
      g_prefix[threadIdx.x] = work->group_prefix[g0 + threadIdx.x];
    }
    __syncthreads();
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
      const unsigned base = (unsigned)tile * kTile + threadIdx.x;
      float first[kPerThread];
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        const unsigned i = base + j * kThreads;
        first[j] = i < S.n_pts ? S.data[FUSED ? (size_t)i : (size_t)i * 3] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < kPerThread; ++j) {
        uint32_t key[3];
        const bool keep = load_keys<FUSED>(S, base + j * kThreads, first[j], key);
        if (PASS == 0) {
#pragma unroll
          for (int a = 0; a < 3; ++a) hist_add(lds + a * kB, key[a] >> digit_shift(0), keep);
        } else {
          for (int s = 0; s < n_here; ++s) {
            const uint32_t ax = g_axis[s], k = ax == 0 ? key[0] : ax == 1 ? key[1] : key[2];
            const bool match = keep && (k >> (digit_shift(PASS) + digit_bits(PASS))) == g_prefix[s];
            hist_add(lds + s * kB, (k >> digit_shift(PASS)) & (kB - 1), match);
          }
        }
      }
    }
    __syncthreads();
    for (int b = (int)threadIdx.x; b < n_here * kB; b += kThreads) {
      const uint32_t v = lds[b];
      if (v) atomicAdd(&hist[(size_t)g0 * kB + b], v);
    }
    __syncthreads();
  }
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) {
  const int lane = (int)(threadIdx.x & 63);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += up;
  }
  return v;
}

// 256 threads = 4 waves; wave w serves targets w, w + 4, ...: lane l sums its run of bins, the wave scans the 64 sums, the
// lane whose run holds the rank walks it
template <int PASS>
__global__ __launch_bounds__(256) void order_stats_narrow_kernel(Work* __restrict__ work, const uint32_t* __restrict__ hist, Quantiles Q,
                                                                 uint32_t* __restrict__ count_out, float* __restrict__ stats) {
  constexpr int kB = 1 << digit_bits(PASS), kRun = kB / 64;
  __shared__ uint32_t t_axis[kMaxTargets], t_prefix[kMaxTargets], t_rank[kMaxTargets];
  const int n_targets = Q.n_q * 6;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const bool live = PASS == 0 || work->n_groups > 0;              // uniform: false when no row was kept
  uint32_t kept = 1;                                              // thread 0 learns the count with target 0
  if (PASS == 0 && (int)threadIdx.x < n_targets) stats[threadIdx.x] = __uint_as_float(0x7FC00000u);
  if (live) {
    for (int t = wave; t < n_targets; t += 4) {
      const uint32_t axis = PASS == 0 ? (uint32_t)((t >> 1) % 3) : min(work->group_axis[min(work->target_group[t], (uint32_t)kMaxTargets - 1)], 2u);
      const uint32_t group = PASS == 0 ? axis : min(work->target_group[t], (uint32_t)kMaxTargets - 1);
      const uint32_t* h = hist + (size_t)group * kB + lane * kRun;
      uint32_t mine = 0;
#pragma unroll
      for (int j = 0; j < kRun; ++j) mine += h[j];
      const uint32_t incl = wave_scan(mine), excl = incl - mine;
      uint32_t rank;
      if (PASS == 0) {
        const uint32_t N = (uint32_t)__shfl((int)incl, 63, 64);   // every axis counts the same rows
        if (t == 0) kept = N;
        if (t == 0 && lane == 0) {
          work->count = N;
          *count_out = N;
        }
        if (N == 0) {
          rank = 0xFFFFFFFFu;                                     // no lane holds it
        } else {
          const double last = (double)(N - 1);
          const double vi = Q.q[t / 6] * last;
          const double lo = fmin(fmax(floor(vi), 0.0), last);
          rank = (uint32_t)((t & 1) ? fmin(lo + 1.0, last) : lo);
        }
      } else {
        rank = work->target_rank[t];
      }
      if (rank >= excl && rank < incl) {
        uint32_t below = excl, bin = 0, left = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < kRun; ++j) {
          const uint32_t c = h[j];
          if (!found && rank < below + c) {
            bin = (uint32_t)j;
            left = rank - below;
            found = true;
          }
          below += c;
        }
        const uint32_t prefix = PASS == 0 ? 0u : work->group_prefix[group];
        t_axis[t] = axis;
        t_prefix[t] = (prefix << digit_bits(PASS)) | (uint32_t)(lane * kRun + bin);
        t_rank[t] = left;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (PASS == 2) {
    if (live)
      for (int t = 0; t < n_targets; ++t) stats[t] = __uint_as_float(bits_of_key(t_prefix[t]));
    return;
  }
  uint32_t n_groups = 0;
  if (live && kept > 0) {
    for (int t = 0; t < n_targets; ++t) {
      uint32_t g = 0;
      while (g < n_groups && !(work->group_axis[g] == t_axis[t] && work->group_prefix[g] == t_prefix[t])) ++g;
      if (g == n_groups) {
        work->group_axis[g] = t_axis[t];
        work->group_prefix[g] = t_prefix[t];
        ++n_groups;
      }
      work->target_group[t] = g;
      work->target_rank[t] = t_rank[t];
    }
  }
  work->n_groups = n_groups;
}

size_t hist_offset(int pass, int n_q) {
  const size_t t = (size_t)n_q * 6;
  size_t off = kHeaderBytes;
  if (pass > 0) off += 3 * (size_t)kBins * 4;
  if (pass > 1) off += t * (size_t)kBins * 4;
  return off;
}

template <bool FUSED>
int run(const char* who, const Source& S, const double* q_host, int n_q, uint32_t* count, float* stats, void* workspace,
        size_t workspace_bytes, hipStream_t s) {
  const size_t need = v3d_order_stats_workspace_bytes(n_q);
  V3D_REQUIRE(workspace_bytes >= need, V3D_ERR_WORKSPACE_TOO_SMALL, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
  V3D_REQUIRE(((uintptr_t)workspace & 7) == 0, V3D_ERR_BAD_ARG, "%s: workspace is not 8-byte aligned", who);
  Quantiles Q;
  Q.n_q = n_q;
  for (int k = 0; k < kMaxQ; ++k) Q.q[k] = k < n_q ? q_host[k] : 0.0;
  Work* work = (Work*)workspace;
  uint32_t* h[3];
  for (int p = 0; p < 3; ++p) h[p] = (uint32_t*)((char*)workspace + hist_offset(p, n_q));
  const int n_tiles = (int)(((long long)S.n_pts + kTile - 1) / kTile);
  const unsigned grid = v3d::persistent_grid(n_tiles, 3);
  V3D_CHECK_HIP(hipMemsetAsync(workspace, 0, need, s));
  {
    v3d::TimedScope scope("order_stats_pass0", s);
    order_stats_pass_kernel<0, FUSED><<<grid, kThreads, 0, s>>>(S, work, h[0], n_tiles);
    V3D_CHECK_LAUNCH("order_stats_pass_kernel<0>");
  }
  order_stats_narrow_kernel<0><<<1, 256, 0, s>>>(work, h[0], Q, count, stats);
  V3D_CHECK_LAUNCH("order_stats_narrow_kernel<0>");
  {
    v3d::TimedScope scope("order_stats_pass1", s);
    order_stats_pass_kernel<1, FUSED><<<grid, kThreads, 0, s>>>(S, work, h[1], n_tiles);
    V3D_CHECK_LAUNCH("order_stats_pass_kernel<1>");
  }
  order_stats_narrow_kernel<1><<<1, 256, 0, s>>>(work, h[1], Q, count, stats);
  V3D_CHECK_LAUNCH("order_stats_narrow_kernel<1>");
  {
    v3d::TimedScope scope("order_stats_pass2", s);
    order_stats_pass_kernel<2, FUSED><<<grid, kThreads, 0, s>>>(S, work, h[2], n_tiles);
    V3D_CHECK_LAUNCH("order_stats_pass_kernel<2>");
  }
  order_stats_narrow_kernel<2><<<1, 256, 0, s>>>(work, h[2], Q, count, stats);
  V3D_CHECK_LAUNCH("order_stats_narrow_kernel<2>");
  return V3D_OK;
}

int check_quantiles(const char* who, const double* q_host, int n_q) {
  V3D_REQUIRE(n_q >= 1 && n_q <= kMaxQ, V3D_ERR_BAD_ARG, "%s: n_q=%d (1 to %d)", who, n_q, kMaxQ);
  V3D_REQUIRE(q_host, V3D_ERR_BAD_ARG, "%s: null argument", who);
  for (int k = 0; k < n_q; ++k)
    V3D_REQUIRE(q_host[k] >= 0.0 && q_host[k] <= 1.0, V3D_ERR_BAD_ARG, "%s: q[%d]=%g (within [0, 1])", who, k, q_host[k]);
  return V3D_OK;
}

}  // namespace

extern "C" size_t v3d_order_stats_workspace_bytes(int n_q) {
  if (n_q < 1 || n_q > kMaxQ) return 0;
  return hist_offset(2, n_q) + (size_t)n_q * 6 * (1 << digit_bits(2)) * 4;
}

extern "C" int v3d_backproject_order_stats_f32(const float* depths, const float* proj_inv, int n, int h, int w, const double* q_host,
                                               int n_q, uint32_t* count, float* stats, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  const char* who = "v3d_backproject_order_stats_f32";
  V3D_REQUIRE(depths && proj_inv && count && stats && workspace, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(n >= 1 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 31) && (long long)n * h * w < (1ll << 31), V3D_ERR_BAD_SHAPE,
              "%s: n=%d h=%d w=%d (positive, fewer than 2^31 pixels)", who, n, h, w);
  const int rc = check_quantiles(who, q_host, n_q);
  if (rc != V3D_OK) return rc;
  Source S;
  S.data = depths;
  S.proj_inv = proj_inv;
  S.n_pts = (unsigned)((long long)n * h * w);
  S.hw = (unsigned)(h * w);
  S.w = (unsigned)w;
  return run<true>(who, S, q_host, n_q, count, stats, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int v3d_cloud_order_stats_f32(const float* pts, int n_pts, const double* q_host, int n_q, uint32_t* count, float* stats,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "v3d_cloud_order_stats_f32";
  V3D_REQUIRE(pts && count && stats && workspace, V3D_ERR_BAD_ARG, "%s: null argument", who);
  V3D_REQUIRE(n_pts >= 1, V3D_ERR_BAD_SHAPE, "%s: n_pts=%d (positive, fewer than 2^31)", who, n_pts);
  const int rc = check_quantiles(who, q_host, n_q);
  if (rc != V3D_OK) return rc;
  Source S;
  S.data = pts;
  S.proj_inv = nullptr;
  S.n_pts = (unsigned)n_pts;
  S.hw = 1;
  S.w = 1;
  return run<false>(who, S, q_host, n_q, count, stats, workspace, workspace_bytes, (hipStream_t)stream);
}
