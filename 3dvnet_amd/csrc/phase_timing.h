// Per-phase cycle counters of a kernel, developer builds only (-DV3D_PHASE_TIMING; scripts/phase_*.py read them): wave 0 of
// every workgroup accumulates the cycles between marks in registers and writes them to its own slot at the end (no atomics:
// they would stall the memory pipe being timed).  Device globals are not shared across translation units in this build, so
// every file that marks phases states PHASE_TIMING_UNIT(reader) once, at file scope behind v3d_common.h and in front of its
// kernels: the file's own slot array and the extern "C" function that sums the slots of the first n_blocks workgroups.
#pragma once
#ifdef V3D_PHASE_TIMING
#include <vector>

constexpr int kPhaseSlots = 1 << 16;
#define PHASE_DECL                                  \
  long long ph_t = __builtin_readcyclecounter();    \
  long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PHASE_MARK(i)                                   \
  do {                                                  \
    long long t_ = __builtin_readcyclecounter();        \
    ph_acc[i] += t_ - ph_t;                             \
    ph_t = t_;                                          \
  } while (0)
#define PHASE_FLUSH                                                                                   \
  do {                                                                                                \
    if (threadIdx.x == 0 && blockIdx.x < kPhaseSlots)                                                 \
      for (int i_ = 0; i_ < 8; ++i_) g_phase[blockIdx.x * 8 + i_] = (unsigned long long)ph_acc[i_];   \
  } while (0)
#define PHASE_TIMING_UNIT(reader)                                                                                    \
  static __device__ unsigned long long g_phase[8 * kPhaseSlots];                                                     \
  extern "C" int reader(unsigned long long* out8_host, int n_blocks) {                                               \
    V3D_CHECK_HIP(hipDeviceSynchronize());                                                                           \
    std::vector<unsigned long long> h((size_t)8 * kPhaseSlots);                                                      \
    V3D_CHECK_HIP(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_phase), h.size() * sizeof(unsigned long long)));        \
    for (int i = 0; i < 8; ++i) out8_host[i] = 0;                                                                    \
    for (int b = 0; b < n_blocks && b < kPhaseSlots; ++b)                                                            \
      for (int i = 0; i < 8; ++i) out8_host[i] += h[(size_t)b * 8 + i];                                              \
    return V3D_OK;                                                                                                   \
  }
#else
#define PHASE_DECL
#define PHASE_MARK(i)
#define PHASE_FLUSH
#define PHASE_TIMING_UNIT(reader)
#endif
