// Hash-indexed sparse-tensor structure kernels replacing MinkowskiEngine's coordinate manager on the
// refinement path (semantics restated in SURVEY Appendix A):
//   * open-addressing hash table over packed (batch, x, y, z) coordinates,
//   * 27-offset neighbour ("kernel map") tables for stride-1 / stride-2 convs and stride-2 transposed
//     convs -- consumed as row maps by the gather-GEMM (gemm_gather.hip).
// The sparse trilinear interpolation on these tables is sparse_interp.hip.
#include "sparse_hash.h"

namespace {

using namespace v3dhash;

__global__ void hash_clear_kernel(HashEntry* entries, unsigned cap, int* status) {
  unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap) entries[i] = HashEntry{kEmpty, -1, 0};
  if (i == 0) *status = 0;
}

__global__ void hash_insert_kernel(HashTable t, const int* __restrict__ coords, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int cb = coords[i * 4], cx = coords[i * 4 + 1], cy = coords[i * 4 + 2], cz = coords[i * 4 + 3];
  if (cb < 0 || cb > 65535 || min(cx, min(cy, cz)) < -kGuard || max(cx, max(cy, cz)) > kCoordMax) {
    atomicOr(t.status, 1);          // would alias another key: reported by v3d_hash_status, row left out
    return;
  }
  const unsigned long long key = pack_key(cb, cx, cy, cz);
  unsigned slot = hash_u64(key) & t.mask;
  for (unsigned probe = 0; probe <= t.mask; ++probe) {
    const unsigned long long prev = atomicCAS(&t.entries[slot].key, kEmpty, key);
    if (prev == kEmpty || prev == key) { t.entries[slot].val = i; return; }   // coordinates are unique rows
    slot = (slot + 1) & t.mask;
  }
}

// nbr[k][p] = row of (out_coords[p] + step * o_k) in the hashed map, o_k in {-1,0,1}^3 with
// k = (ox+1) + 3 (oy+1) + 9 (oz+1);  conv: step = +ts_in, transposed conv: step = -ts_out.
// One thread per (offset, output row): the 27 probes of a row were a loop in one thread -- 27 dependent probe chains in a row,
// 40-50 us per launch whatever the level's size (2.8 k rows took as long as 60 k).  blockIdx.y = offset k, so a wave's stores
// are 64 consecutive ints of column k.
__global__ void neighbors_kernel(HashTable t, const int* __restrict__ out_coords, int n_out, int step,
                                 int* __restrict__ nbr) {
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (i >= n_out) return;
  const int4 c = *reinterpret_cast<const int4*>(out_coords + (size_t)i * 4);      // (batch, x, y, z)
  const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;
  nbr[(size_t)k * n_out + i] = hash_find(t, pack_key(c.x, c.y + step * ox, c.z + step * oy, c.w + step * oz));
}

}  // namespace

extern "C" size_t v3d_hash_bytes(int n) { return (size_t)table_capacity(n) * sizeof(HashEntry) + 16; }

extern "C" int v3d_hash_status(const void* table, int n, void* stream) {
  V3D_REQUIRE(table && n > 0, V3D_ERR_BAD_ARG, "v3d_hash_status: bad argument");
  HashTable t = table_view(const_cast<void*>(table), n);
  int st = 0;
  V3D_CHECK_HIP(hipMemcpyAsync(&st, t.status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  V3D_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  V3D_REQUIRE(st == 0, V3D_ERR_BAD_SHAPE,
              "v3d_hash_build: a coordinate is outside the packed-key range (batch 0..65535, x/y/z %d..%d)", -kGuard,
              kCoordMax);
  return V3D_OK;
}

extern "C" int v3d_hash_build(const int32_t* coords, int n, void* table, size_t table_bytes, void* stream) {
  V3D_REQUIRE(coords && table, V3D_ERR_BAD_ARG, "v3d_hash_build: null argument");
  V3D_REQUIRE(n > 0, V3D_ERR_BAD_SHAPE, "v3d_hash_build: empty coordinate map");
  V3D_REQUIRE(table_bytes >= v3d_hash_bytes(n), V3D_ERR_WORKSPACE_TOO_SMALL, "v3d_hash_build: table buffer too small");
  hipStream_t s = (hipStream_t)stream;
  HashTable t = table_view(table, n);
  v3d::TimedScope ts("hash_build", s);
  hash_clear_kernel<<<(t.mask + 256) / 256, 256, 0, s>>>(t.entries, t.mask + 1, t.status);
  hash_insert_kernel<<<(n + 255) / 256, 256, 0, s>>>(t, coords, n);
  V3D_CHECK_LAUNCH("hash_insert_kernel");
  return V3D_OK;
}

extern "C" int v3d_sparse_neighbors(const void* table, int n_in, const int32_t* out_coords, int n_out,
                                    int step, int32_t* nbr, void* stream) {
  V3D_REQUIRE(table && out_coords && nbr, V3D_ERR_BAD_ARG, "v3d_sparse_neighbors: null argument");
  V3D_REQUIRE(n_in > 0 && n_out > 0 && step != 0, V3D_ERR_BAD_SHAPE, "v3d_sparse_neighbors: bad shape");
  V3D_REQUIRE((reinterpret_cast<size_t>(out_coords) & 15) == 0, V3D_ERR_BAD_ARG,
              "v3d_sparse_neighbors: out_coords must be 16-byte aligned (the kernel loads a coordinate row as one int4)");
  hipStream_t s = (hipStream_t)stream;
  HashTable t = table_view(const_cast<void*>(table), n_in);
  v3d::TimedScope ts("sparse_neighbors", s);
  neighbors_kernel<<<dim3((n_out + 255) / 256, 27), 256, 0, s>>>(t, out_coords, n_out, step, nbr);
  V3D_CHECK_LAUNCH("neighbors_kernel");
  return V3D_OK;
}
