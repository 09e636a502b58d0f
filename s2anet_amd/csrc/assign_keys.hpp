// Label assignment: the pieces the per-image op and the batched op (both assign_ops.hip) must share to give
// the same ids -- the order-preserving integer key of an overlap and the anchor validity rule.
#pragma once
#include <hip/hip_runtime.h>

namespace s2a {

// overlap -> int key, monotone for v >= 0 (atomicMax on keys == max on overlaps); every filtered (negative) overlap is 0
__device__ __forceinline__ int iou_key(float v) { return v < 0.f ? 0 : __float_as_int(v) + 1; }
__device__ __forceinline__ float key_iou(int k) { return k == 0 ? -0.5f : __int_as_float(k - 1); }

__device__ __forceinline__ bool anchor_valid(const float* __restrict__ a, float img_h, float img_w) {
  return a[0] >= 0 && a[1] >= 0 && a[0] <= img_w && a[1] <= img_h && a[2] < img_w && a[3] < img_h;   // :63-69
}

}  // namespace s2a
