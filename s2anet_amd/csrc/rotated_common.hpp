// What more than one of rotated_ops.hip (NMS, candidate compaction), iou_ops.hip (box IoU) and assign_ops.hip (label
// assignment) uses, and nothing else: a symbol with one user lives in that user's file.  Internal to the library.
//
// Everything but SideSet sits in the anonymous namespace, as the kernels of every translation unit here do: the library
// builds without relocatable device code, so each object gets its own copy of what it includes (k_fill_u32 is a plain
// kernel and is emitted into every object that includes this header, used or not).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace s2a {
namespace {

constexpr int kThreads = 256;
constexpr int kPersistentGrid = 1024;
constexpr int kIouCap = 8;               // candidate-point slots per lane of the fast exact-IoU passes (rbox_iou)
constexpr int kHeavyGrid = 2048;         // 8 workgroups per CU

// bits of a measurement / ablation build of the including object (s2a_build_flags(), common.cpp): every translation unit
// reports its own through a build_flags_*() function
constexpr int kBuildFlags = 0
#ifdef S2A_MEASURE
                            | 1
#endif
#ifdef S2A_ABL_NOFENCE
                            | 2
#endif
    ;

// ---------------------------------------------------------------- workgroup pair queue
struct PairQueue {
  uint2* q;            // LDS: kLdsQueue (NMS) / kIouQueue (box IoU) entries
  unsigned* count;     // LDS
  unsigned* base;      // LDS (flush broadcast)
};

__device__ __forceinline__ void queue_push(PairQueue& Q, unsigned i, unsigned j) {
  unsigned p = atomicAdd(Q.count, 1u);
  Q.q[p] = make_uint2(i, j);
}

// all threads of the workgroup call this; copies the LDS queue to the global list
__device__ __forceinline__ void queue_flush(PairQueue& Q, uint2* __restrict__ gq,
                                            unsigned long long* __restrict__ gcount,
                                            unsigned long long cap) {
  __syncthreads();
  unsigned cnt = *Q.count;
  if (cnt == 0) return;  // uniform
  if (threadIdx.x == 0) {
    unsigned long long b = atomicAdd(gcount, (unsigned long long)cnt);
    Q.base[0] = (unsigned)(b & 0xffffffffu);
    Q.base[1] = (unsigned)(b >> 32);
  }
  __syncthreads();
  unsigned long long b = ((unsigned long long)Q.base[1] << 32) | Q.base[0];
  for (unsigned e = threadIdx.x; e < cnt; e += blockDim.x) {
    unsigned long long dst = b + e;
    if (dst < cap) gq[dst] = Q.q[e];  // beyond cap: dropped, gcount keeps the true total
  }
  __syncthreads();
  if (threadIdx.x == 0) *Q.count = 0;
  __syncthreads();
}

// Hand-off of LDS data between the lanes of ONE wave (no workgroup barrier): the hardware issues a wave's LDS
// operations in order, so all that is needed is that the COMPILER keeps the order too.  Wavefront-scope fences + the wave
// barrier emit no instruction; they pin the order of the LDS stores / atomics before against the LDS loads after.
__device__ __forceinline__ void wave_lds_handoff() {
#ifdef S2A_ABL_NOFENCE
  return;
#endif
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// small fills by a kernel: hipMemsetAsync nodes of a captured graph were not replayed correctly (ROCm 7.2; see nms_core)
__global__ void k_fill_u32(uint32_t* __restrict__ p, uint32_t v, size_t count) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = v;
}
inline void fill_u32(void* p, uint32_t v, size_t count, hipStream_t st) {
  if (count) k_fill_u32<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(static_cast<uint32_t*>(p), v, count);
}

}  // namespace

// Two side streams + fork / join events of one (device, caller stream); the registry that hands them out exists once per
// process: side_set(), declared in common.hpp, defined in rotated_ops.hip
struct SideSet {
  int dev = -1;
  hipStream_t caller = nullptr;
  hipStream_t s[2] = {nullptr, nullptr};
  hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
};

}  // namespace s2a
