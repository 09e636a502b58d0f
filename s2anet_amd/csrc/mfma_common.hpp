// Pieces shared by the two MFMA translation units, dcn_ops.hip (deformable conv / AlignConv) and conv_ops.hip (dense f16
// convolutions): vector types, the LDS row pitch, position-tile and XCD index maps, and the pyramid level table.
// Everything sits in an unnamed namespace: each translation unit gets its own copy (the project builds without relocatable
// device code).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace s2a {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

constexpr int kRowBytes = 144;  // LDS row: 128 B of K data + 16 B pad (conflict-free b128 reads)

// 2-D position tiles: a workgroup owns a 16-wide x (NPOS/16)-high patch of one image, so the
// footprint of its bilinear corners (patch + halo) is a few hundred pixels instead of a whole
// image row.  Returns the linear position b*H*W + y*W + x, or -1 outside the image / batch.
__device__ __forceinline__ int64_t tile_pos(int64_t tile, int pl, int th, int H, int W, int64_t HW,
                                            int64_t Ntot) {
  const int txn = (W + 15) / 16, tyn = (H + th - 1) / th;
  const int64_t b = tile / (txn * tyn);
  const int r = (int)(tile % (txn * tyn));
  const int y = (r / txn) * th + (pl >> 4), xq = (r % txn) * 16 + (pl & 15);
  const int64_t g = b * HW + (int64_t)y * W + xq;
  return (y < H && xq < W && g < Ntot) ? g : -1;
}

// XCD-aware tile order: blockIdx round-robins over the 8 XCDs (private L2 each); give every XCD
// a contiguous run of position tiles so neighbouring tiles (which sample overlapping input rows)
// share one L2.  Bijective for any tile count (cdna guide T1).
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned n) {
  const unsigned q = n / 8, r = n % 8, x = bid % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + bid / 8;
}

// Pyramid-packed launches: the FPN levels of one head layer share their filters, so all of them go
// through ONE launch.  The levels sit back to back in one NHWC buffer (level l = [B,H_l,W_l,C] at
// pixel offset pix0[l]); a workgroup finds its level from the tile index and rebinds its pointers
// and geometry -- from there on it is an ordinary single-level tile.  n <= 1: plain tensor.
constexpr int kMaxLevels = 8;
struct LevelTab {
  int n, batch;
  int H[kMaxLevels], W[kMaxLevels], tile0[kMaxLevels], pix0[kMaxLevels];
  float stride[kMaxLevels];
};

// tiles (tile_rows x 16 positions) per level, pixel offsets; returns the total tile count or -1
inline int64_t build_levels(const s2a_pyramid* pyr, int64_t batch, LevelTab* lt, int64_t* total_pix, int tile_rows = 8) {
  if (!pyr || pyr->n_levels < 1 || pyr->n_levels > kMaxLevels) return -1;
  *lt = LevelTab{};
  lt->n = pyr->n_levels;
  lt->batch = (int)batch;
  int64_t tiles = 0, pix = 0;
  for (int i = 0; i < pyr->n_levels; i++) {
    const int64_t H = pyr->height[i], W = pyr->width[i];
    if (H < 1 || W < 1 || H >= 32000 || W >= 32000) return -1;
    lt->H[i] = (int)H; lt->W[i] = (int)W; lt->stride[i] = pyr->stride[i];
    lt->tile0[i] = (int)tiles; lt->pix0[i] = (int)pix;
    tiles += batch * ((W + 15) / 16) * ((H + tile_rows - 1) / tile_rows);
    pix += batch * H * W;
    if (tiles >= (1ll << 31) || pix >= (1ll << 31)) return -1;
  }
  *total_pix = pix;
  return tiles;
}

}  // namespace
}  // namespace s2a
