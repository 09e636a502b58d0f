// Deformable convolution v1 forward / AlignConv for MI355X (gfx950).
//
// Replaces:
//   deform_conv_forward_cuda        models/dcn/src/deform_conv_cuda.cpp:152-260
//   deformable_im2col_gpu_kernel    models/dcn/src/deform_conv_cuda_kernel.cu:189-242
//   deformable_im2col_bilinear      models/dcn/src/deform_conv_cuda_kernel.cu:83-114
//   AlignConv.get_offset / forward  models/alignconv.py:30-98
//
// The reference materialises a [C*9, B*H*W] `columns` matrix in HBM (1.2 GB at P3, B=8),
// zero-fills it, writes it with an uncoalesced NCHW gather and re-reads it in a cuBLAS GEMM.
// Here the op is ONE kernel per call and `columns` never exists:
//   * activations are read channels-last (NHWC): a bilinear corner is a contiguous run of
//     channels, so every gather instruction moves full 128-byte lines
//   * a workgroup owns 64 output positions x all (<=256) output channels; per (tap, channel
//     chunk) stage it gathers + blends the column tile straight into LDS and streams the
//     matching pre-packed weight tile into LDS
//   * the contraction runs on the matrix cores: v_mfma_f32_32x32x2_f32 (exact f32 FMA chain,
//     1e-4 parity with the f32 reference) or v_mfma_f32_32x32x16_f16 (f16 in, f32 accumulate)
//   * LDS tiles are double-buffered (one barrier per stage): next stage's global loads are
//     in flight under the current stage's MFMAs
//   * sampling coordinates come either from the reference's [B,18,H,W] offset tensor or —
//     AlignConv fused — directly from the refined anchors (the 18-channel tensor is never
//     written), with ReLU fused into the epilogue
// Sampling semantics (border rule h_im > -1 && < H, corner dropping, weight order) follow
// deform_conv_cuda_kernel.cu:97-112,:228 exactly.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "mfma_common.hpp"

namespace s2a {
namespace {

#ifndef S2A_STAMP
#define S2A_STAMP 0
#endif
#ifndef S2A_STAMP_W2
#define S2A_STAMP_W2 4        // second stamped wave (0 is the first)
#endif
#if S2A_STAMP
// diagnostic build only: per-workgroup phase stamps (s_memtime) into a buffer nothing else reads
__device__ unsigned long long g_stamps[4096 * 16];
#define S2A_STAMP_AT(slot)                                                                   \
  do {                                                                                       \
    if (lane == 0 && (wave == 0 || wave == S2A_STAMP_W2))                                    \
      g_stamps[((blockIdx.x & 4095) * 16) + (wave ? 8 : 0) + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#define S2A_TIC() (t_tic = __builtin_amdgcn_s_memtime())
#define S2A_TOC(accv) (accv += __builtin_amdgcn_s_memtime() - t_tic)
#define S2A_STAMP_VAL(slot, val)                                                             \
  do {                                                                                       \
    if (lane == 0 && (wave == 0 || wave == S2A_STAMP_W2))                                    \
      g_stamps[((blockIdx.x & 4095) * 16) + (wave ? 8 : 0) + (slot)] = (val);                \
  } while (0)
#else
#define S2A_STAMP_AT(slot) do {} while (0)
#define S2A_TIC() do {} while (0)
#define S2A_TOC(accv) do {} while (0)
#define S2A_STAMP_VAL(slot, val) do {} while (0)
#endif

constexpr int kMaxO = 256;      // output channels per workgroup

// ------------------------------------------------------------------ layout helpers
template <typename T>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const T* __restrict__ src, int64_t B, int C,
                                                      int64_t HW, T* __restrict__ dst) {
  // 32x32 tile transpose through LDS: reads coalesced along HW, writes coalesced along C
  __shared__ T tile[32][33];
  const int64_t b = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    int c = c0 + r;
    int64_t p = p0 + tx;
    if (c < C && p < HW) tile[r][tx] = src[(b * C + c) * HW + p];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    int64_t p = p0 + r;
    int c = c0 + tx;
    if (c < C && p < HW) dst[(b * HW + p) * C + c] = tile[tx][r];
  }
}

// weight [O][C][9] -> packed [C/KC][9][O][KC]  (KC = channels per stage; stage s = cc*9 + tap:
// the 9 taps of one channel chunk run back to back, so their overlapping corner pixels stay in L1)
template <typename T>
__global__ void k_pack_weight(const T* __restrict__ w, int O, int C, int KC, T* __restrict__ wp) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)O * C * 9;
  if (e >= total) return;
  int k = (int)(e % KC);
  int64_t r = e / KC;
  int o = (int)(r % O);
  r /= O;
  int t = (int)(r % 9);
  int cc = (int)(r / 9);
  wp[e] = w[((int64_t)o * C + cc * KC + k) * 9 + t];
}

// ------------------------------------------------------------------ sampling table
struct Tap {
  int idx[4];   // global pixel index (b*H*W + h*W + w) of the 4 corners, 0 when dropped
  float w[4];   // bilinear weights hh*hw, hh*lw, lh*hw, lh*lw; 0 when dropped / outside
};

__device__ __forceinline__ Tap make_tap(float h_im, float w_im, int H, int W, int64_t img_pix0) {
  Tap t;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    t.idx[k] = (int)img_pix0;
    t.w[k] = 0.f;
  }
  if (h_im > -1 && w_im > -1 && h_im < H && w_im < W) {  // kernel.cu:228
    int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
    int h_high = h_low + 1, w_high = w_low + 1;
    float lh = h_im - h_low, lw = w_im - w_low;
    float hh = 1 - lh, hw = 1 - lw;
    if (h_low >= 0 && w_low >= 0) {
      t.idx[0] = (int)(img_pix0 + (int64_t)h_low * W + w_low);
      t.w[0] = hh * hw;
    }
    if (h_low >= 0 && w_high <= W - 1) {
      t.idx[1] = (int)(img_pix0 + (int64_t)h_low * W + w_high);
      t.w[1] = hh * lw;
    }
    if (h_high <= H - 1 && w_low >= 0) {
      t.idx[2] = (int)(img_pix0 + (int64_t)h_high * W + w_low);
      t.w[2] = lh * hw;
    }
    if (h_high <= H - 1 && w_high <= W - 1) {
      t.idx[3] = (int)(img_pix0 + (int64_t)h_high * W + w_high);
      t.w[3] = lh * lw;
    }
  }
  return t;
}

// sampling point of tap (ky,kx) at output (y,x), 3x3 / stride 1 / pad 1 / dilation 1
struct AnchorCtx {
  float x_ctr, y_ctr, dw, dh, cs, sn;
};
__device__ __forceinline__ AnchorCtx anchor_ctx(const float* a, float stride) {
  // models/alignconv.py:58-62
  AnchorCtx c;
  c.x_ctr = a[0] / stride;
  c.y_ctr = a[1] / stride;
  float w = a[2] / stride, h = a[3] / stride;
  c.cs = cosf(a[4]);
  c.sn = sinf(a[4]);
  c.dw = w / 3.0f;
  c.dh = h / 3.0f;
  return c;
}
__device__ __forceinline__ void anchor_offset(const AnchorCtx& c, int ky, int kx, float yc, float xc,
                                              float& off_y, float& off_x) {
  // models/alignconv.py:63-70 (same operation order as s2a_align_offsets)
  float xx = (float)(kx - 1), yy = (float)(ky - 1);
  float x = c.dw * xx, y = c.dh * yy;
  float xr = c.cs * x - c.sn * y;
  float yr = c.sn * x + c.cs * y;
  off_x = (xr + c.x_ctr) - (xc + xx);
  off_y = (yr + c.y_ctr) - (yc + yy);
}

// ------------------------------------------------------------------ fused MFMA kernel
template <typename T>
struct Traits;
template <>
struct Traits<float> {
  static constexpr int KC = 32;      // channels per stage (128 B per corner)
  static constexpr int VEC = 4;      // elements per 16-B vector
};
template <>
struct Traits<_Float16> {
  static constexpr int KC = 64;
  static constexpr int VEC = 8;
};

template <typename T>
struct Vec16;
template <>
struct Vec16<float> {
  using type = f32x4;
};
template <>
struct Vec16<_Float16> {
  using type = f16x8;
};

template <typename T>
__device__ __forceinline__ typename Vec16<T>::type blend(const typename Vec16<T>::type (&v)[4],
                                                         const float (&w)[4]);
template <>
__device__ __forceinline__ f32x4 blend<float>(const f32x4 (&v)[4], const float (&w)[4]) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; e++) r[e] = w[0] * v[0][e] + w[1] * v[1][e] + w[2] * v[2][e] + w[3] * v[3][e];
  return r;
}
template <>
__device__ __forceinline__ f16x8 blend<_Float16>(const f16x8 (&v)[4], const float (&w)[4]) {
  f16x8 r;
#pragma unroll
  for (int e = 0; e < 8; e++)
    r[e] = (_Float16)(w[0] * (float)v[0][e] + w[1] * (float)v[1][e] + w[2] * (float)v[2][e] +
                      w[3] * (float)v[3][e]);
  return r;
}

// f16 blend in packed half arithmetic (v_pk_mul/v_pk_fma_f16): the reference's half path
// evaluates w1*v1 + w2*v2 + w3*v3 + w4*v4 in scalar_t = half as well (kernel.cu:110-112)
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
__device__ __forceinline__ f16x8 blend_pk(const f16x8 (&v)[4], const float (&w)[4]) {
  f16x8 r;
  f16x2 w0 = {(_Float16)w[0], (_Float16)w[0]}, w1 = {(_Float16)w[1], (_Float16)w[1]};
  f16x2 w2 = {(_Float16)w[2], (_Float16)w[2]}, w3 = {(_Float16)w[3], (_Float16)w[3]};
#pragma unroll
  for (int e = 0; e < 4; e++) {
    f16x2 a0 = {v[0][2 * e], v[0][2 * e + 1]}, a1 = {v[1][2 * e], v[1][2 * e + 1]};
    f16x2 a2 = {v[2][2 * e], v[2][2 * e + 1]}, a3 = {v[3][2 * e], v[3][2 * e + 1]};
    // explicit FMAs: with plain `w1 * a1 + acc` the compiler is free to fuse EITHER product of a sum of two products
    // into the add, and picks differently between instantiations (1-ulp differences between tile shapes)
    f16x2 acc = w0 * a0;
    acc = __builtin_elementwise_fma(w1, a1, acc);
    acc = __builtin_elementwise_fma(w2, a2, acc);
    acc = __builtin_elementwise_fma(w3, a3, acc);
    r[2 * e] = acc[0];
    r[2 * e + 1] = acc[1];
  }
  return r;
}

// the same blend with the four weights still in binary16 (the sampling table stores them so): no conversions
__device__ __forceinline__ f16x8 blend_pk_h(const f16x8 (&v)[4], const _Float16 (&w)[4]) {
  f16x8 r;
  const f16x2 w0 = {w[0], w[0]}, w1 = {w[1], w[1]}, w2 = {w[2], w[2]}, w3 = {w[3], w[3]};
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const f16x2 a0 = {v[0][2 * e], v[0][2 * e + 1]}, a1 = {v[1][2 * e], v[1][2 * e + 1]};
    const f16x2 a2 = {v[2][2 * e], v[2][2 * e + 1]}, a3 = {v[3][2 * e], v[3][2 * e + 1]};
    f16x2 acc = w0 * a0;
    acc = __builtin_elementwise_fma(w1, a1, acc);
    acc = __builtin_elementwise_fma(w2, a2, acc);
    acc = __builtin_elementwise_fma(w3, a3, acc);
    r[2 * e] = acc[0];
    r[2 * e + 1] = acc[1];
  }
  return r;
}

// SRC: 0 = offset tensor [B,18,H,W] f32, 1 = refined anchors [B,H,W,5] f32
// NPOS: output positions per workgroup (64: more workgroups for small inputs; 128: the weight tile
// is amortised over twice the positions)
template <typename T, bool OUT_NHWC, int SRC, int NPOS>
__global__ __launch_bounds__(256, 1) void k_dcn_mfma(const T* __restrict__ x,       // NHWC
                                                     const float* __restrict__ src,  // offsets | anchors
                                                     const T* __restrict__ wp,       // packed weights
                                                     T* __restrict__ out, int64_t Ntot, int C, int H,
                                                     int W, int O, float stride, int relu) {
  constexpr int KC = Traits<T>::KC;
  constexpr int VEC = Traits<T>::VEC;
  constexpr int NT = NPOS / 32;    // 32-wide position tiles per wave
  constexpr int ITEMS = NPOS / 32; // (position, 16-byte channel group) items per thread
  using V = typename Vec16<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [ taps NPOS*9*32 B | A0 | B0 | A1 | B1 ]
  Tap* s_tab = reinterpret_cast<Tap*>(smem);
  constexpr int kTabBytes = NPOS * 9 * 32;
  constexpr int kABytes = kMaxO * kRowBytes, kBBytes = NPOS * kRowBytes;
  char* s_buf = smem + kTabBytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t HW = (int64_t)H * W;
  const int64_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int o0 = blockIdx.y * kMaxO;
  const int Oloc = min(kMaxO, O - o0);
  const int CC = C / KC;
  const int nstage = 9 * CC;

  // ---- sampling table for this tile
  for (int e = tid; e < NPOS * 9; e += 256) {
    int pl = e / 9, t = e % 9;
    int64_t g = tile_pos(tile, pl, NPOS / 16, H, W, HW, Ntot);
    Tap tp;
    if (g >= 0) {
      int64_t b = g / HW, p = g % HW;
      int y = (int)(p / W), xq = (int)(p % W);
      int ky = t / 3, kx = t % 3;
      float off_y, off_x;
      if (SRC == 0) {
        const float* ob = src + (b * 18) * HW + p;
        off_y = ob[(int64_t)(2 * t) * HW];
        off_x = ob[(int64_t)(2 * t + 1) * HW];
      } else {
        AnchorCtx c = anchor_ctx(src + g * 5, stride);
        anchor_offset(c, ky, kx, (float)y, (float)xq, off_y, off_x);
      }
      float h_im = (float)(y - 1 + ky) + off_y;  // kernel.cu:226-227
      float w_im = (float)(xq - 1 + kx) + off_x;
      tp = make_tap(h_im, w_im, H, W, b * HW);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        tp.idx[k] = 0;
        tp.w[k] = 0.f;
      }
    }
    s_tab[e] = tp;
  }
  __syncthreads();

  f32x16 acc[2][NT];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  // per-thread staging registers
  V cv[ITEMS][4];
  float cw[ITEMS][4];
  V av[8];

  auto issue = [&](int s) {
    const int t = s % 9, cc = s / 9;
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      int item = tid + 256 * it;
      int pl = item >> 3, q = item & 7;
      const Tap tp = s_tab[pl * 9 + t];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        cw[it][k] = tp.w[k];
        // a dropped corner (outside the image: weight 0, index of the image's first pixel) is not loaded: 0 * inf is NaN
        cv[it][k] = tp.w[k] != 0.f ? *reinterpret_cast<const V*>(x + (int64_t)tp.idx[k] * C + cc * KC + q * VEC) : V{};
      }
    }
    const T* wsrc = wp + ((int64_t)s * O + o0) * KC;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      int idx = tid + 256 * r;
      int row = idx >> 3, q = idx & 7;
      if (row < Oloc) av[r] = *reinterpret_cast<const V*>(wsrc + (int64_t)row * KC + q * VEC);
    }
  };
  auto commit = [&](int buf) {
    char* A = s_buf + buf * (kABytes + kBBytes);
    char* Bm = A + kABytes;
#pragma unroll
    for (int it = 0; it < ITEMS; it++) {
      int item = tid + 256 * it;
      int pl = item >> 3, q = item & 7;
      if constexpr (sizeof(T) == 2)
        *reinterpret_cast<V*>(Bm + pl * kRowBytes + q * 16) = blend_pk(cv[it], cw[it]);
      else
        *reinterpret_cast<V*>(Bm + pl * kRowBytes + q * 16) = blend<T>(cv[it], cw[it]);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
      int idx = tid + 256 * r;
      int row = idx >> 3, q = idx & 7;
      if (row < Oloc) *reinterpret_cast<V*>(A + row * kRowBytes + q * 16) = av[r];
    }
  };

  issue(0);
  commit(0);
  __syncthreads();

  const bool wave_active = wave * 64 < Oloc;
  for (int s = 0; s < nstage; s++) {
    const int buf = s & 1;
    if (s + 1 < nstage) issue(s + 1);
    if (wave_active) {
      const char* A = s_buf + buf * (kABytes + kBBytes);
      const char* Bm = A + kABytes;
      const char* wrow = A + (wave * 64 + (lane & 31)) * kRowBytes + (lane >> 5) * 16;
      const char* prow = Bm + (lane & 31) * kRowBytes + (lane >> 5) * 16;
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
        V wf[2], pf[NT];
#pragma unroll
        for (int h = 0; h < 2; h++) wf[h] = *reinterpret_cast<const V*>(wrow + h * 32 * kRowBytes + kk * 32);
#pragma unroll
        for (int h = 0; h < NT; h++) pf[h] = *reinterpret_cast<const V*>(prow + h * 32 * kRowBytes + kk * 32);
        if constexpr (sizeof(T) == 4) {
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
              for (int b = 0; b < NT; b++) {
                if constexpr (OUT_NHWC)
                  acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(pf[b][j], wf[a][j], acc[a][b], 0, 0, 0);
                else
                  acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[a][j], pf[b][j], acc[a][b], 0, 0, 0);
              }
        } else {
#pragma unroll
          for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < NT; b++) {
              if constexpr (OUT_NHWC)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf[b], wf[a], acc[a][b], 0, 0, 0);
              else
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[a], pf[b], acc[a][b], 0, 0, 0);
            }
        }
      }
    }
    if (s + 1 < nstage) commit(buf ^ 1);
    __syncthreads();
  }

  if (!wave_active) return;
  // ---- epilogue: ReLU + store.  acc[a][b] = (out-channel tile a, position tile b);
  // MFMA D layout: column = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = acc[a][b][r];
        if (relu) v = fmaxf(v, 0.f);
        int rowi = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if constexpr (OUT_NHWC) {
          // operands swapped: rows = positions, columns = out channels (128 B runs along channels)
          int64_t g = tile_pos(tile, 32 * b + rowi, NPOS / 16, H, W, HW, Ntot);
          int och = o0 + wave * 64 + 32 * a + (lane & 31);
          if (g >= 0) out[g * O + och] = (T)v;
        } else {
          int och = o0 + wave * 64 + 32 * a + rowi;
          int64_t g = tile_pos(tile, 32 * b + (lane & 31), NPOS / 16, H, W, HW, Ntot);
          if (g >= 0) {
            int64_t bi = g / HW, p = g % HW;
            out[(bi * O + och) * HW + p] = (T)v;
          }
        }
      }
}

// ------------------------------------------------------------------ patch-staged variant (f16)
// The vector-memory path of a CU sustains only ~30 B/clk for 16-B-per-lane gathers (measured on the
// wave-specialised global gather that preceded this kernel: its loader side took 3.3 k cycles per
// stage even with every load dropped by a zero-record descriptor), and the 9 taps of one position
// re-read almost the same pixels.  So:
//   * the input patch around the 8x16 position tile (16x24 pixels x 64 channels = 48 KB) is
//     loaded ONCE per channel chunk into LDS; the 9 taps gather their corners from LDS
//     (ds_read_b128, ~10x the bandwidth of the global gather); corners outside the patch fall
//     back to global loads (rare for anchor-sized offsets)
//   * the weight tile never touches LDS: it is pre-packed in MFMA-fragment order and every MFMA
//     wave loads its own 8 KB per stage straight into registers (1 KB contiguous per instruction),
//     one stage ahead — which frees 72 KB of LDS for the double-buffered patch
// L1 traffic per stage drops from 96 KB to ~38 KB.
struct alignas(16) PTap {
  short y, x;        // top-left bilinear corner (h_low, w_low), image coordinates
  unsigned flags;    // bit 0: all four corners lie inside the LDS patch
  _Float16 w[4];     // hh*hw, hh*lw, lh*hw, lh*lw; 0 where the corner is dropped
};
constexpr int kPH = 16, kPW = 24, kHalo = 4;
constexpr int kPatchBytes = kPH * kPW * 128;
constexpr int kPatchLds = 128 * 9 * 16 + 2 * 128 * kRowBytes + 2 * kPatchBytes;  // 153600 B

// weight [O][C][9] f16 for the 16x16x32 matrix waves of k_dcn_patch: [stage = cc*9+t][och group of 64][fragment f = 2a + ks (8)][lane 64][8 halfs],
// lane = (i = lane & 15, kg = lane >> 4): element j = W[g*64 + och_l(a, i)][cc*64 + 32 (kg & 1) + 16 ks + 8 (kg >> 1) + j][t] with
// och_l(a, i) = 32 (a >> 1) + 8 (i >> 2) + 4 (a & 1) + (i & 3).  One contiguous 1 KB load per fragment, and the D rows of a lane
// (4 kg + e of fragments a = 0..3) are out channels 8 kg .. 8 kg + 7 and 32 + 8 kg .. 32 + 8 kg + 7 of its pixel: the epilogue
// stores two 16-byte vectors per pixel straight from the accumulators (no LDS staging, no barrier)
__device__ __forceinline__ int frag16_och(int a, int i) { return 32 * (a >> 1) + 8 * (i >> 2) + 4 * (a & 1) + (i & 3); }
__global__ void k_pack_weight_frag16(const _Float16* __restrict__ w, int O, int C, _Float16* __restrict__ wp) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)O * C * 9;
  if (e >= total) return;
  const int G = O / 64;
  int j = (int)(e & 7);
  int lane = (int)((e >> 3) & 63);
  int f = (int)((e >> 9) & 7);
  int64_t r = e >> 12;
  int g = (int)(r % G);
  int st = (int)(r / G);
  int t = st % 9, cc = st / 9;
  int och = g * 64 + frag16_och(f >> 1, lane & 15);
  int k = cc * 64 + 32 * ((lane >> 4) & 1) + 16 * (f & 1) + 8 * (lane >> 5) + j;   // the k slots of the column fragments (bfrag)
  wp[e] = w[((int64_t)och * C + k) * 9 + t];
}

// TH = rows of the position tile: 8 (128 positions), or 4 (64 positions: half tiles for launches that fill the chip badly,
// e.g. one P3 level of one chip = 128 full tiles on 256 CUs; tile index = tile_base + block / 2, half = block & 1)
// (MW = 4 matrix waves, one per SIMD, 64 out channels x all positions each.  The form with EIGHT -- two per SIMD, 32 out channels
// each, twelve waves of <= 168 registers, the later patch chunks in two halves -- passed the same tests and measured 10 % slower,
// 241.7 against 219.8 us: DESIGN 4)
template <bool OUT_NHWC, int SRC, int TH = 8>
__device__ __forceinline__ void dcn_patch_tile(const _Float16* __restrict__ x_,
                                               const float* __restrict__ src_,
                                               const _Float16* __restrict__ wfrag,
                                               _Float16* __restrict__ out_, int64_t Ntot_, int C,
                                               int H_, int W_, int O, float stride_, int relu,
                                               unsigned x_bytes_, const LevelTab& lt, int tile_base, unsigned vb, unsigned nvb, const int tid) {
  using T = _Float16;
  using V = f16x8;
  constexpr int NPOS = TH * 16, NT = NPOS / 32, ITEMS = NPOS / 32;
  constexpr int kPHt = TH + 2 * kHalo;                 // patch rows
  constexpr int kPatchBytesT = kPHt * kPW * 128;
  constexpr int NPV = kPHt * kPW * 8 / 256;            // 16-byte patch vectors per loader thread (12 | 9)
  static_assert(TH == 8 || TH == 4, "tile height");
  constexpr int MW = 4, NTHR = 64 * (MW + 4);          // matrix waves (0 .. MW-1; the loaders are waves MW .. MW+3), threads
  constexpr int AH = 16 / MW;                          // 16-channel accumulator tiles per matrix wave
  static_assert(kPHt * kPW * 8 % 256 == 0, "patch vectors must divide among the loader threads");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PTap* s_tab = reinterpret_cast<PTap*>(smem);
  char* s_B = smem + NPOS * 9 * 16;
  char* s_patch = s_B + 2 * NPOS * kRowBytes;

  const bool half_coords = (relu & 2) != 0;          // relu: bit 0 = ReLU epilogue, bit 1 = S2A_DCN_HALF_COORDS
  auto rh16 = [](float v) { return (float)(_Float16)v; };
  const int lane = tid & 63, wave = tid >> 6;                      // (waves 0-3 = matrix: the older half wins issue
                                                                   // arbitration; roles swapped measured 4 % slower)
  int64_t tile = xcd_remap(vb, nvb);
  const int half = TH == 4 ? (int)(tile & 1) : 0;
  if (TH == 4) tile >>= 1;
  tile += tile_base;
  const T* x = x_;
  const float* src = src_;
  T* out = out_;
  int64_t Ntot = Ntot_;
  int H = H_, W = W_;
  float stride = stride_;
  unsigned x_bytes = x_bytes_;
  if (SRC == 1 && lt.n > 1) {         // pyramid-packed levels (anchors [sum B*H*W, 5] packed alike)
    int t0 = 0, p0 = 0;
#pragma unroll
    for (int i = 0; i < kMaxLevels; i++)
      if (i < lt.n && tile >= lt.tile0[i]) {
        t0 = lt.tile0[i]; p0 = lt.pix0[i]; H = lt.H[i]; W = lt.W[i]; stride = lt.stride[i];
      }
    tile -= t0;
    Ntot = (int64_t)lt.batch * H * W;
    x += (int64_t)p0 * C;
    out += (int64_t)p0 * O;
    src += (int64_t)p0 * 5;
    x_bytes = (unsigned)(Ntot * C * 2);
  }
  const int64_t HW = (int64_t)H * W;
  const int txn = (W + 15) / 16, tyn = (H + 7) / 8;
  const int64_t bimg = tile / (txn * tyn);
  const int trem = (int)(tile % (txn * tyn));
  const int ty0 = (trem / txn) * 8 + 4 * half, tx0 = (trem % txn) * 16;
  const int oy = ty0 - kHalo, ox = tx0 - kHalo;
  const int o0 = blockIdx.y * kMaxO;
  const int Oloc = min(kMaxO, O - o0);
  const int CC = C / 64;
  const int nstage = 9 * CC;
  const int G = O / 64;
  const unsigned row_bytes = (unsigned)C * 2;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, (int)x_bytes, 0x00020000);

  S2A_STAMP_AT(0);
  S2A_STAMP_VAL(6, __builtin_amdgcn_s_memrealtime());   // (matrix wave; 100 MHz: the in-kernel clock is d memtime / d memrealtime)
  // ---- loader waves: put the first patch in flight before anything else (its latency hides
  // under the table build).  patch element v = L + 256*i: pixel v>>3, 16-byte channel group v&7;
  // out-of-image pixels get an out-of-range offset -> the bounds-checked load returns zeros.
  const int L = tid - 64 * MW;
  auto patch_off = [&](int i) -> unsigned {
    int v = L + 256 * i, p = v >> 3, q = v & 7;
    int yy = oy + p / kPW, xx = ox + p % kPW;
    bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    return in ? (unsigned)((bimg * HW + (int64_t)yy * W + xx) * row_bytes + q * 16) : 0x80000000u;
  };
  unsigned pvoff[NPV];
  V pv[NPV];
  if (wave >= MW) {
#pragma unroll
    for (int i = 0; i < NPV; i++) {
      const unsigned o = patch_off(i);
      pvoff[i] = o;
      u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)o, 0, 0);
      pv[i] = __builtin_bit_cast(V, d);
    }
  }

  // ---- MFMA waves: first weight fragments in flight now as well (one memory latency for the
  // whole prologue instead of three in a row)
  const int g = min(o0 / 64 + (wave & 3), G - 1);
  const V* wf_base = reinterpret_cast<const V*>(wfrag) + lane;
  constexpr int WR = 2;                                // filter fragments per matrix wave and stage: 4 WR
  V wA[WR][4], wB[WR][4];
  // 16x16x32 MFMAs (lane maps and the reason: k_conv_f16; the 32x32x16 form of rounds 1-2 measured +1.7 %).
  // Lane = (i = lane & 15, kg = lane >> 4); fragment f = (16-channel tile f >> 1, k-step f & 1) in k_pack_weight_frag16
  // order; 16-position tile pt = tile row pt, its pixel for lane i = pix16 (conflict-free ds_read_b128 on the 144-byte
  // rows of the column tile)
  const int kg16 = lane >> 4, i16 = lane & 15;
  const int pix16 = (i16 >= 4 && i16 < 12) ? (((i16 - 4) >> 1) * 4 + (i16 & 1))
                                           : (((i16 & 3) >> 1) * 4 + 2 + (i16 & 1) + (i16 >= 12 ? 8 : 0));
  auto load_w = [&](int s, V (&wv)[WR][4]) {
    const V* p = wf_base + ((int64_t)s * G + g) * 8 * 64;        // k_pack_weight_frag16 order: 1 KB per fragment
#pragma unroll
    for (int f = 0; f < 4 * WR; f++) wv[f >> 2][f & 3] = p[f * 64];
  };
  if (wave < MW) load_w(0, wA);

  // ---- one table entry: tap t of tile position pl, anchor context c (SRC 1) or the offset maps (SRC 0)
  auto table_entry = [&](int pl, int t, const AnchorCtx& c) {
    int y = ty0 + (pl >> 4), xq = tx0 + (pl & 15);
    PTap tp;
    tp.y = (short)oy;
    tp.x = (short)ox;
    tp.flags = 1u;
#pragma unroll
    for (int k = 0; k < 4; k++) tp.w[k] = (_Float16)0.f;
    if (y < H && xq < W) {
      const int64_t p = (int64_t)y * W + xq;
      int ky = t / 3, kx = t % 3;
      float off_y, off_x;
      if (SRC == 0) {
        const float* ob = src + (bimg * 18) * HW + p;
        off_y = ob[(int64_t)(2 * t) * HW];
        off_x = ob[(int64_t)(2 * t + 1) * HW];
      } else {
        anchor_offset(c, ky, kx, (float)y, (float)xq, off_y, off_x);
      }
      // half_coords: the reference's scalar_t = Half instantiation (deform_conv.py:45-46 casts the offsets to half;
      // deform_conv_cuda_kernel.cu:221-228 h_im / w_im, :97-109 lh / lw / hh / hw and the four weights are Half
      // results): every one of them rounded to binary16.  Default: f32 coordinates.  ONE uniform branch per
      // entry: written as a rounding after each step the compiler computed both forms and selected per value
      // (30 of the entry's 150 instructions for a mode that is off)
      float h_im, w_im, lh = 0.f, lw = 0.f, hh = 0.f, hw = 0.f;
      int h_low = 0, w_low = 0;
      bool inside;
      if (!half_coords) {
        h_im = (float)(y - 1 + ky) + off_y;
        w_im = (float)(xq - 1 + kx) + off_x;
        inside = h_im > -1 && w_im > -1 && h_im < H && w_im < W;
        if (inside) {
          h_low = (int)floorf(h_im); w_low = (int)floorf(w_im);
          lh = h_im - h_low; lw = w_im - w_low;
          hh = 1 - lh; hw = 1 - lw;
        }
      } else {
        off_y = rh16(off_y); off_x = rh16(off_x);
        h_im = rh16((float)(y - 1 + ky) + off_y);
        w_im = rh16((float)(xq - 1 + kx) + off_x);
        inside = h_im > -1 && w_im > -1 && h_im < H && w_im < W;
        if (inside) {
          h_low = (int)floorf(h_im); w_low = (int)floorf(w_im);
          lh = rh16(h_im - h_low); lw = rh16(w_im - w_low);
          hh = rh16(1 - lh); hw = rh16(1 - lw);
        }
      }
      if (inside) {
        bool t_ok = h_low >= 0, b_ok = h_low + 1 <= H - 1, l_ok = w_low >= 0, r_ok = w_low + 1 <= W - 1;
        tp.w[0] = (_Float16)((t_ok && l_ok) ? hh * hw : 0.f);
        tp.w[1] = (_Float16)((t_ok && r_ok) ? hh * lw : 0.f);
        tp.w[2] = (_Float16)((b_ok && l_ok) ? lh * hw : 0.f);
        tp.w[3] = (_Float16)((b_ok && r_ok) ? lh * lw : 0.f);
        tp.y = (short)h_low;
        tp.x = (short)w_low;
        bool in = h_low >= oy && h_low + 1 <= oy + kPHt - 1 && w_low >= ox && w_low + 1 <= ox + kPW - 1;
        // bits 31..1: byte offset of the top-left corner inside a patch buffer (clamped for corners that left the
        // patch: those items are redone from global memory) -- the loader adds it instead of re-deriving it per stage
        const int py = min(max(h_low - oy, 0), kPHt - 2), px = min(max(w_low - ox, 0), kPW - 2);
        tp.flags = (in ? 1u : 0u) | ((unsigned)((py * kPW + px) * 128) << 1);
      }
    }
    s_tab[pl * 9 + t] = tp;
  };
  // ---- per-position anchor context (cos/sin once per position, not once per tap).  It lives in the SECOND column buffer:
  // the first one is written (first column tile) while the matrix waves still read contexts for the rest of the table
  AnchorCtx* s_ctx = reinterpret_cast<AnchorCtx*>(s_B + NPOS * kRowBytes);
  static_assert(NPOS * sizeof(AnchorCtx) <= NPOS * kRowBytes, "contexts fit a column buffer");
  if (SRC == 1 && tid < NPOS) {
    int y = ty0 + (tid >> 4), xq = tx0 + (tid & 15);
    AnchorCtx c = {0, 0, 0, 0, 1, 0};
    if (y < H && xq < W) c = anchor_ctx(src + (bimg * HW + (int64_t)y * W + xq) * 5, stride);
    s_ctx[tid] = c;
  }
  if (SRC == 1) __syncthreads();

  // ---- sampling table, TAP-major (entry e = tap e / NPOS of position e % NPOS): everyone builds the first NTHR entries
  // (taps 0 .. 3 of a full tile), which is all the loaders need for their first column tiles; the matrix waves, idle until
  // the first columns exist, build the rest under the loaders' first tile (the whole table in front of barrier #1 was
  // 2.85 k cycles with the matrix pipes and then the loaders waiting on each other: 9.9 k cycles before the first MFMA)
  auto table_entries = [&](int e0, int e1, int t0, int nthr) {
    for (int e = e0 + t0; e < e1; e += nthr) {
      const int pl = e % NPOS, t = e / NPOS;
      AnchorCtx c = {0, 0, 0, 0, 1, 0};
      if (SRC == 1) c = s_ctx[pl];
      table_entry(pl, t, c);
    }
  };
  constexpr int kTabFirst = NTHR < NPOS * 9 ? NTHR : NPOS * 9;        // 512 entries = taps 0 .. 3 (TH 8), 0 .. 7 (TH 4)
  static_assert(kTabFirst % NPOS == 0 && kTabFirst / NPOS >= 2, "the first round of entries covers whole taps, at least taps 0 and 1");
  table_entries(0, kTabFirst, tid, NTHR);
  if (wave >= MW) {  // first patch -> LDS
#pragma unroll
    for (int i = 0; i < NPV; i++) *reinterpret_cast<V*>(s_patch + (L + 256 * i) * 16) = pv[i];
  }
  S2A_STAMP_AT(1);
  __syncthreads();  // #1 table rows of the first taps + patch 0 ready
  S2A_STAMP_AT(2);
  if (wave < MW) table_entries(kTabFirst, NPOS * 9, tid, 64 * MW);   // (s_ctx is dead behind barrier #2)

  f32x4 acc16[AH][2 * NT];
  const bool wave_active = wave < MW && (wave & 3) * 64 < Oloc;
  if (wave < MW) {
    // ===================== MFMA waves =====================
#pragma unroll
    for (int a = 0; a < AH; a++)
#pragma unroll
      for (int b = 0; b < 2 * NT; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc16[a][b][r] = 0.f;
    const int last = nstage - 1;
    __syncthreads();  // #2 stage 0 columns in LDS
    S2A_STAMP_AT(3);
    int s = 0;
    unsigned long long t_tic = 0, t_work = 0, t_wait = 0;
    (void)t_tic; (void)t_work; (void)t_wait;
    // B fragments one k-step AHEAD of the MFMAs that use them (two register sets), also across the stage boundary: the
    // stage's barrier sits in front of the LAST k-step, after all four reads of the current tile have been issued and
    // have landed -- behind it the next tile is sealed and its first fragments are requested under the last 2*NT MFMAs.
    // (The plain form read 2 k-steps and waited for them at once: two exposed LDS round trips per stage plus one behind
    // the barrier.)  Same MFMAs in the same order: bit-identical.
    V p0[NT], p1[NT];
    // (no branch on wave_active in here: a wave without out-channels computes on clamped filter fragments and drops the
    // result in the epilogue -- a branch would split the basic block and hipcc's waitcnt pass then waits for ALL LDS
    // reads at every join, the prefetched ones included)
    // step kk = (k-step kk >> 1 of 32 channels, half kk & 1 of the wave's 16-position tiles): NT reads and 4 NT MFMAs of
    // 16 cycles per step
    auto bfrag = [&](int st, int kk, V (&pf)[NT]) {
      const char* prow = s_B + (st & 1) * (NPOS * kRowBytes) + ((kk & 1) * NT * 16 + pix16) * kRowBytes + (kg16 & 1) * 64 + (kg16 >> 1) * 16 + (kk >> 1) * 32;
#pragma unroll
      for (int h = 0; h < NT; h++) pf[h] = *reinterpret_cast<const V*>(prow + h * 16 * kRowBytes);
    };
    auto mma = [&](const V (&wv)[WR][4], int kk, const V (&pf)[NT]) {
      const int ks = kk >> 1, bh = (kk & 1) * NT;
#pragma unroll
      for (int a = 0; a < AH; a++)
#pragma unroll
        for (int b = 0; b < NT; b++)
          acc16[a][bh + b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[(a * 2 + ks) >> 2][(a * 2 + ks) & 3], pf[b], acc16[a][bh + b], 0, 0, 0);
    };
    auto stage = [&](int st, const V (&wv)[WR][4]) {
      bfrag(st, 1, p1); __builtin_amdgcn_sched_barrier(0);
      mma(wv, 0, p0);   __builtin_amdgcn_sched_barrier(0);
      bfrag(st, 2, p0); __builtin_amdgcn_sched_barrier(0);
      mma(wv, 1, p1);   __builtin_amdgcn_sched_barrier(0);
      bfrag(st, 3, p1); __builtin_amdgcn_sched_barrier(0);
      mma(wv, 2, p0);   __builtin_amdgcn_sched_barrier(0);
      __syncthreads();  // tile st+1 sealed; this tile's buffer is free for the loaders (all its reads have landed)
      bfrag(min(st + 1, last), 0, p0); __builtin_amdgcn_sched_barrier(0);   // (last stage: a dead re-read)
      mma(wv, 3, p1);   __builtin_amdgcn_sched_barrier(0);
    };
    bfrag(0, 0, p0);
    for (; s + 1 < nstage; s += 2) {
      load_w(s + 1, wB);
      stage(s, wA);
      load_w(min(s + 2, last), wA);
      stage(s + 1, wB);
    }
    if (s < nstage) stage(s, wA);
  } else {
    // ===================== loader waves =====================
    auto patch_issue = [&](int cc) {
#pragma unroll
      for (int i = 0; i < NPV; i++) {
        u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)pvoff[i], cc * 128, 0);
        pv[i] = __builtin_bit_cast(V, d);
      }
    };
    auto patch_write = [&](int cc) {
      char* P = s_patch + (cc & 1) * kPatchBytesT;
#pragma unroll
      for (int i = 0; i < NPV; i++) *reinterpret_cast<V*>(P + (L + 256 * i) * 16) = pv[i];
    };
    // The operands of a stage (4 table entries, 16 corner vectors per thread) are FETCHED one stage ahead -- right
    // after the previous stage's columns have been written, so their LDS latency (table read, then the dependent
    // corner reads) runs under the barrier wait instead of in front of the blend.
    PTap tp[ITEMS];
    V c[ITEMS][4];
    auto fetch = [&](int s) {
      const int t = s % 9, cc = s / 9;
      const char* P = s_patch + (cc & 1) * kPatchBytesT + (L & 7) * 16;   // (item & 7 = L & 7 for every item)
#pragma unroll
      for (int it = 0; it < ITEMS; it++)      // one 16-byte read per entry
        tp[it] = __builtin_bit_cast(PTap, *reinterpret_cast<const u32x4*>(&s_tab[((L + 256 * it) >> 3) * 9 + t]));
#pragma unroll
      for (int it = 0; it < ITEMS; it++) {
        // out-of-patch items read a clamped (wrong) location here and are redone in produce()
        const char* b0 = P + (tp[it].flags >> 1);
        c[it][0] = *reinterpret_cast<const V*>(b0);
        c[it][1] = *reinterpret_cast<const V*>(b0 + 128);
        c[it][2] = *reinterpret_cast<const V*>(b0 + kPW * 128);
        c[it][3] = *reinterpret_cast<const V*>(b0 + kPW * 128 + 128);
      }
    };
    auto produce = [&](int s) {  // columns of stage s (operands fetched before) -> B[s&1]
      const int cc = s / 9;
      char* Bm = s_B + (s & 1) * (NPOS * kRowBytes);
      bool any_out = false;
#pragma unroll
      for (int it = 0; it < ITEMS; it++) any_out |= !(tp[it].flags & 1u);
#pragma unroll
      for (int it = 0; it < ITEMS; it++) {
        const int item = L + 256 * it, pl = item >> 3, q = item & 7;
        const float cw[4] = {(float)tp[it].w[0], (float)tp[it].w[1], (float)tp[it].w[2], (float)tp[it].w[3]};
        *reinterpret_cast<V*>(Bm + pl * kRowBytes + q * 16) = blend_pk(c[it], cw);
      }
      if (any_out) {  // rare: a corner left the patch -> global gather for that (position, tap)
        for (int it = 0; it < ITEMS; it++) {
          if (tp[it].flags & 1u) continue;
          const int item = L + 256 * it, pl = item >> 3, q = item & 7;
          V g4[4];
#pragma unroll
          for (int k = 0; k < 4; k++) {
            int yy = min(max((int)tp[it].y + (k >> 1), 0), H - 1), xx = min(max((int)tp[it].x + (k & 1), 0), W - 1);
            unsigned vo = (unsigned)((bimg * HW + (int64_t)yy * W + xx) * row_bytes + q * 16);
            u32x4 d = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)vo, cc * 128, 0);
            g4[k] = __builtin_bit_cast(V, d);
          }
          const float cw[4] = {(float)tp[it].w[0], (float)tp[it].w[1], (float)tp[it].w[2], (float)tp[it].w[3]};
          *reinterpret_cast<V*>(Bm + pl * kRowBytes + q * 16) = blend_pk(g4, cw);
        }
      }
    };

    if (CC > 1) patch_issue(1);
    fetch(0);
    produce(0);
    if (nstage > 1) fetch(1);
    S2A_STAMP_AT(6);
    __syncthreads();  // #2 stage 0 columns in LDS
    S2A_STAMP_AT(3);
    unsigned long long t_tic = 0, t_work = 0, t_wait = 0;
    (void)t_tic; (void)t_work; (void)t_wait;
    for (int s = 0; s < nstage; s++) {
      const int sn = s + 1;          // stage produced while stage s is consumed
      S2A_TIC();
      if (sn < nstage) {
        const int t = sn % 9, cc = sn / 9;
        if (t == 4 && cc + 1 < CC) patch_write(cc + 1);   // loads issued >= 3 stages ago
        produce(sn);
        if (t == 8 && cc + 2 < CC) patch_issue(cc + 2);   // next-next chunk: lands during the next chunk
        if (sn + 1 < nstage) fetch(sn + 1);               // (chunk of stage sn+1: written >= 4 stages ago)
      }
      S2A_TOC(t_work); S2A_TIC();
      __syncthreads();
      S2A_TOC(t_wait);
    }
    S2A_STAMP_VAL(7, t_work);
    S2A_STAMP_VAL(5, t_wait);   // (loader slot 5 = 13 overall; its end stamp is not used)
  }

  S2A_STAMP_AT(4);
  // ===================== epilogue =====================
  auto out_pos = [&](int pos) -> int64_t {       // linear position b*H*W + y*W + x of tile position pos, -1 outside
    const int y = ty0 + (pos >> 4), xq = tx0 + (pos & 15);
    const int64_t gpos = bimg * HW + (int64_t)y * W + xq;
    return (y < H && xq < W && gpos < Ntot) ? gpos : -1;
  };
  if constexpr (OUT_NHWC) {
    // straight from the accumulators (filter rows permuted by k_pack_weight_frag16): lane (pixel pix16 of 16-position tile b,
    // kg16) holds out channels 8 kg16 .. +7 (fragments 0, 1) and 32 + 8 kg16 .. +7 (fragments 2, 3) of its wave's 64 -- two
    // 16-byte stores per pixel, no LDS staging, no barrier (the LDS-staged whole-row form measured +1 %).
    // ReLU on the rounded halves, two per instruction (rounding is monotonic and keeps zero and sign: max(round(v), 0) ==
    // round(max(v, 0)); a NaN becomes 0 either way), and the ReLU switch as ONE uniform branch around the tile: with
    // fmaxf + a per-value select on the f32 accumulators the epilogue was 800 instructions, 5.3 k of a tile's 87 k cycles
    auto store_tile = [&](auto relu_c) {
      constexpr bool kRelu = decltype(relu_c)::value;
      using h2 = __attribute__((ext_vector_type(2))) _Float16;
      // tile position 16 b + pix16 = (row ty0 + b, column tx0 + pix16): one address, then a row pitch per b
      auto pack8 = [&](int b, int hf) {
        V v8;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const f32x4& a4 = acc16[2 * hf + (i >> 1)][b];
          h2 v = {(_Float16)a4[2 * (i & 1)], (_Float16)a4[2 * (i & 1) + 1]};
          if constexpr (kRelu) v = __builtin_elementwise_max(v, h2{(_Float16)0.f, (_Float16)0.f});
          v8[2 * i] = v[0];
          v8[2 * i + 1] = v[1];
        }
        return v8;
      };
      const int xq = tx0 + pix16;
      int64_t gp = bimg * HW + (int64_t)ty0 * W + xq;
      _Float16* orow = out + o0 + (wave & 3) * 64 + 8 * kg16 + gp * O;
      const int64_t pitch = (int64_t)W * O;
#pragma unroll
      for (int b = 0; b < 2 * NT; b++, gp += W, orow += pitch) {
        const bool ok = xq < W && ty0 + b < H && gp < Ntot;
#pragma unroll
        for (int hf = 0; hf < AH / 2; hf++)
          if (ok) *reinterpret_cast<V*>(orow + 32 * hf) = pack8(b, hf);
      }
    };
    if (wave_active) {
      if (relu & 1) store_tile(std::true_type{}); else store_tile(std::false_type{});
    }
    S2A_STAMP_AT(5);
    if (wave == 0) S2A_STAMP_VAL(7, __builtin_amdgcn_s_memrealtime());
  } else {
    if (!wave_active) return;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 2 * NT; b++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
          float v = acc16[a][b][e];
          if (relu & 1) v = fmaxf(v, 0.f);
          const int och = o0 + wave * 64 + 32 * (a >> 1) + 8 * kg16 + 4 * (a & 1) + e;
          const int64_t gp = out_pos(16 * b + pix16);
          if (gp >= 0) {
            int64_t bi = gp / HW, p = gp % HW;
            out[(bi * O + och) * HW + p] = (T)v;
          }
        }
  }
}

// the launch.  n_full = 0: one TH-row tile per workgroup.  n_full > 0 (TH 8 only): workgroups [0, n_full) take full 8 x 16
// tiles, the workgroups behind them take the remaining tiles as 4 x 16 HALF tiles (two per tile) -- the hardware hands out
// workgroups in index order, so the halves are what runs last.  Why: the launch is rounds of one workgroup per CU, every round
// as long as a tile (36.7 us), and the last round of the detector's pyramid holds 84 tiles for 256 CUs: as 168 half tiles
// (0.62 of a tile each) it costs 0.62 rounds instead of one.  (A fixed grid of workgroups walking the tiles in a loop -- with
// the arguments re-read and the thread index laundered per tile so that nothing is hoisted across the body -- was bit-identical
// and 3 % SLOWER, 227 against 220 us: it keeps the same 6-tile critical path and adds a barrier per tile.)
struct PatchArgs {
  const _Float16* x;
  const float* src;
  const _Float16* wfrag;
  _Float16* out;
  int64_t Ntot;
  int C, H, W, O;
  float stride;
  int relu;
  unsigned x_bytes;
  int tile_base;
  unsigned n_full;
  LevelTab lt;
};
template <bool OUT_NHWC, int SRC, int TH = 8>
__global__ __launch_bounds__(512, 2) void k_dcn_patch(PatchArgs a) {
  if constexpr (TH == 8 && OUT_NHWC && SRC == 1) {
    if (a.n_full != 0 && blockIdx.x >= a.n_full) {      // (uniform)
      dcn_patch_tile<OUT_NHWC, SRC, 4>(a.x, a.src, a.wfrag, a.out, a.Ntot, a.C, a.H, a.W, a.O, a.stride, a.relu, a.x_bytes, a.lt,
                                           (int)a.n_full, blockIdx.x - a.n_full, gridDim.x - a.n_full, threadIdx.x);
      return;
    }
  }
  dcn_patch_tile<OUT_NHWC, SRC, TH>(a.x, a.src, a.wfrag, a.out, a.Ntot, a.C, a.H, a.W, a.O, a.stride, a.relu, a.x_bytes, a.lt,
                                        a.tile_base, blockIdx.x, a.n_full ? a.n_full : gridDim.x, threadIdx.x);
}

// CU count of the CURRENT device (cached per device index: a process may drive devices of different size)
inline int device_cu_count(int* out) {
  static int cached[64] = {};
  int dev = 0;
  S2A_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || cached[dev] == 0) {
    hipDeviceProp_t prop;
    S2A_HIP(hipGetDeviceProperties(&prop, dev));
    const int n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (dev >= 0 && dev < 64) __atomic_store_n(&cached[dev], n, __ATOMIC_RELAXED);   // (racing writers store the same value)
    *out = n;
    return S2A_OK;
  }
  *out = cached[dev];
  return S2A_OK;
}

// ------------------------------------------------------------------ f32 AlignConv / deformable conv on the 16-bit matrix instruction
// The f32 matrix instruction runs at 1/16 of the 16-bit rate (k_dcn_mfma<float>: 0.55 of ITS peak = 225 us for one
// [1,256,128,128] level).  An f32 value is EXACTLY the sum of three bf16 values (hi = rne(x), mid = rne(x - hi), lo = rne(x - hi -
// mid): 8 + 8 + 8 significand bits), and a product without its three smallest cross terms is six bf16 products accumulated
// in f32 (|error| <~ 3 * 2^-24 of the product: one f32 rounding) -- six v_mfma_f32_32x32x16_bf16 for eight 32x32x2 f32 ones of
// a quarter their length.  k_dcn_x3 is k_dcn_mfma's dataflow with that arithmetic: per stage (tap, 16 input channels) the
// four bilinear corners of every position are gathered from the NHWC input, blended in f32 (im2col_bilinear's order) and
// written to LDS as three bf16 planes; the filter was split into its planes when it was packed (k_pack_weight_x3); the waves
// read both operands with ds_read_b128 (48-byte rows: conflict-free) and run 6 MFMAs per output tile and stage.
// S2A_DCN_F32=mfma32 selects the f32 instruction's kernel (A/B, and the tests' cross-check).
constexpr int kX3KC = 16;                       // input channels per stage = one k-step of 32x32x16
constexpr int kX3Row = 48;                      // bytes per LDS row: 16 bf16 + 16 B pad (12 dwords: sixteen rows start in sixteen 4-bank groups)
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;
template <int NPOS>
constexpr int x3_lds_bytes() { return NPOS * 9 * 32 + 2 * 3 * (kMaxO + NPOS) * kX3Row; }      // 110 592 / 147 456
// weight [O][C][9] f32 -> [stage s = (c / 16) * 9 + tap][plane][O][16] bf16
__global__ void k_pack_weight_x3(const float* __restrict__ w, int O, int C, __bf16* __restrict__ wp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)O * C * 9) return;
  const int t = (int)(e % 9);
  const int64_t oc = e / 9;
  const int c = (int)(oc % C), o = (int)(oc / C);
  const int64_t st = (int64_t)(c / kX3KC) * 9 + t;
  __bf16 h, m, l;
  split3(w[e], h, m, l);
  const int64_t base = (st * 3 * O + o) * kX3KC + (c % kX3KC), plane = (int64_t)O * kX3KC;
  wp[base] = h;
  wp[base + plane] = m;
  wp[base + 2 * plane] = l;
}

template <bool OUT_NHWC, int SRC, int NPOS>
__global__ __launch_bounds__(512, 1) void k_dcn_x3(const float* __restrict__ x,       // NHWC
                                                   const float* __restrict__ src,     // offsets | anchors
                                                   const __bf16* __restrict__ wp,     // k_pack_weight_x3
                                                   float* __restrict__ out, int64_t Ntot, int C, int H,
                                                   int W, int O, float stride, int relu) {
  // eight waves, two per SIMD (one wave's blend / split / requests run under the other's MFMAs): wave = (64-out-channel group
  // wave & 3, position half wave >> 2)
  constexpr int NT = NPOS / 64;        // 32-wide position tiles per wave
  constexpr int kItems = NPOS * 4;     // (position, 4-channel group) items per stage: one per thread (NPOS 64: threads 0-255)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [ taps NPOS*9*32 B | A0 (3 planes) | B0 (3 planes) | A1 | B1 ]
  Tap* s_tab = reinterpret_cast<Tap*>(smem);
  constexpr int kTabBytes = NPOS * 9 * 32;
  constexpr int kAPlane = kMaxO * kX3Row, kBPlane = NPOS * kX3Row;
  constexpr int kBufBytes = 3 * (kAPlane + kBPlane);
  char* s_buf = smem + kTabBytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, phalf = tid >> 8;
  const int64_t HW = (int64_t)H * W;
  const int64_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int o0 = blockIdx.y * kMaxO;
  const int Oloc = min(kMaxO, O - o0);
  const int CC = C / kX3KC;
  const int nstage = 9 * CC;

  // ---- sampling table for this tile (as k_dcn_mfma)
  for (int e = tid; e < NPOS * 9; e += 512) {
    int pl = e / 9, t = e % 9;
    int64_t g = tile_pos(tile, pl, NPOS / 16, H, W, HW, Ntot);
    Tap tp;
    if (g >= 0) {
      int64_t b = g / HW, p = g % HW;
      int y = (int)(p / W), xq = (int)(p % W);
      int ky = t / 3, kx = t % 3;
      float off_y, off_x;
      if (SRC == 0) {
        const float* ob = src + (b * 18) * HW + p;
        off_y = ob[(int64_t)(2 * t) * HW];
        off_x = ob[(int64_t)(2 * t + 1) * HW];
      } else {
        AnchorCtx c = anchor_ctx(src + g * 5, stride);
        anchor_offset(c, ky, kx, (float)y, (float)xq, off_y, off_x);
      }
      float h_im = (float)(y - 1 + ky) + off_y;  // kernel.cu:226-227
      float w_im = (float)(xq - 1 + kx) + off_x;
      tp = make_tap(h_im, w_im, H, W, b * HW);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        tp.idx[k] = 0;
        tp.w[k] = 0.f;
      }
    }
    s_tab[e] = tp;
  }
  __syncthreads();

  f32x16 acc[2][NT];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  // per-thread staging registers, TWO sets: one wave per SIMD runs a stage's 24-48 MFMAs in 0.8-1.5 k cycles, less than an L2
  // round trip under load, so a stage's requests go out TWO stages ahead (one stage ahead: 202 us for one [1,256,128,128]
  // level against 227 on the f32 instruction; the matrix work is 46 us)
  struct Stage {
    f32x4 cv[4];
    float cw[4];
    bf16x8 av[3];                      // 3 planes x 256 rows x two 16-byte halves = 1 536 vectors
  };
  Stage ra, rb;

  auto issue = [&](int s, Stage& r_) {
    const int t = s % 9, cc = s / 9;
    if (tid < kItems) {
      const int pl = tid >> 2, q = tid & 3;
      const Tap tp = s_tab[pl * 9 + t];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        r_.cw[k] = tp.w[k];
        // (a dropped corner is not loaded: see k_dcn_mfma)
        r_.cv[k] = tp.w[k] != 0.f ? *reinterpret_cast<const f32x4*>(x + (int64_t)tp.idx[k] * C + cc * kX3KC + q * 4) : f32x4{};
      }
    }
    const __bf16* wsrc = wp + (int64_t)s * 3 * O * kX3KC;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      int idx = tid + 512 * r;
      int plane = idx >> 9, row = (idx & 511) >> 1, q = idx & 1;
      if (row < Oloc) r_.av[r] = *reinterpret_cast<const bf16x8*>(wsrc + ((int64_t)plane * O + o0 + row) * kX3KC + q * 8);
    }
  };
  auto commit = [&](int buf, const Stage& r_) {
    char* A = s_buf + buf * kBufBytes;
    char* Bm = A + 3 * kAPlane;
    if (tid < kItems) {
      const int pl = tid >> 2, q = tid & 3;
      const f32x4 v = blend<float>(r_.cv, r_.cw);
      bf16x4 h, m, l;
#pragma unroll
      for (int j = 0; j < 4; j++) { __bf16 a, b2, c; split3(v[j], a, b2, c); h[j] = a; m[j] = b2; l[j] = c; }
      char* d = Bm + pl * kX3Row + q * 8;
      *reinterpret_cast<bf16x4*>(d) = h;
      *reinterpret_cast<bf16x4*>(d + kBPlane) = m;
      *reinterpret_cast<bf16x4*>(d + 2 * kBPlane) = l;
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      int idx = tid + 512 * r;
      int plane = idx >> 9, row = (idx & 511) >> 1, q = idx & 1;
      if (row < Oloc) *reinterpret_cast<bf16x8*>(A + plane * kAPlane + row * kX3Row + q * 16) = r_.av[r];
    }
  };

  const bool wave_active = wave * 64 < Oloc;
  auto mfma_stage = [&](int buf) {
    if (!wave_active) return;
    const char* A = s_buf + buf * kBufBytes;
    const char* Bm = A + 3 * kAPlane;
    const char* wrow = A + (wave * 64 + (lane & 31)) * kX3Row + (lane >> 5) * 16;
    const char* prow = Bm + (phalf * NT * 32 + (lane & 31)) * kX3Row + (lane >> 5) * 16;
    bf16x8 wf[3][2], pf[3][NT];
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
      for (int h = 0; h < 2; h++) wf[p][h] = *reinterpret_cast<const bf16x8*>(wrow + p * kAPlane + h * 32 * kX3Row);
#pragma unroll
      for (int h = 0; h < NT; h++) pf[p][h] = *reinterpret_cast<const bf16x8*>(prow + p * kBPlane + h * 32 * kX3Row);
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < NT; b++) {
        // (filter plane, column plane): the three small terms first
        constexpr int kPw[6] = {2, 0, 1, 1, 0, 0}, kPp[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int k = 0; k < 6; k++) {
          if constexpr (OUT_NHWC)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[kPp[k]][b], wf[kPw[k]][a], acc[a][b], 0, 0, 0);
          else
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[kPw[k]][a], pf[kPp[k]][b], acc[a][b], 0, 0, 0);
        }
      }
  };
  // stage s: requests of stage s + 2 (into the set stage s used), MFMAs of stage s, operands of stage s + 1 into the other buffer.
  // Measured and not kept (batch 8 / one image, 914 / 142 us as shipped): the two waves of a SIMD taking the halves of a stage in
  // opposite order (one blends while the other holds the matrix pipe) 973 / 140 -- the branch doubles the loop body; stages tap
  // by tap with the corner addresses hoisted (nine table reads per tile instead of 144) 984 / 156 -- chunk by chunk the nine
  // taps of a 16-channel chunk re-touch the same 64-byte pieces of neighbouring pixels while they are still in the L1.
  auto step = [&](int s, Stage& r_issue, const Stage& r_commit) {
    if (s + 2 < nstage) issue(s + 2, r_issue);
    mfma_stage(s & 1);
    if (s + 1 < nstage) commit((s + 1) & 1, r_commit);
    __syncthreads();
  };
  issue(0, ra);
  if (nstage > 1) issue(1, rb);
  commit(0, ra);
  __syncthreads();
  for (int s = 0; s < nstage; s += 2) {
    step(s, ra, rb);
    if (s + 1 < nstage) step(s + 1, rb, ra);
  }

  if (!wave_active) return;
  // ---- epilogue: ReLU + store.  acc[a][b] = (out-channel tile a, position tile b);
  // MFMA D layout: column = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = acc[a][b][r];
        if (relu) v = fmaxf(v, 0.f);
        int rowi = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if constexpr (OUT_NHWC) {
          int64_t g = tile_pos(tile, 32 * (phalf * NT + b) + rowi, NPOS / 16, H, W, HW, Ntot);
          int och = o0 + wave * 64 + 32 * a + (lane & 31);
          if (g >= 0) out[g * O + och] = v;
        } else {
          int och = o0 + wave * 64 + 32 * a + rowi;
          int64_t g = tile_pos(tile, 32 * (phalf * NT + b) + (lane & 31), NPOS / 16, H, W, HW, Ntot);
          if (g >= 0) {
            int64_t bi = g / HW, p = g % HW;
            out[(bi * O + och) * HW + p] = v;
          }
        }
      }
}

template <int NPOS>
constexpr int mfma_lds_bytes() { return NPOS * 9 * 32 + 2 * (kMaxO + NPOS) * kRowBytes; }  // 110592 / 147456

// ------------------------------------------------------------------ generic fallback
// Any stride / padding / dilation / groups / deformable groups / channel count, NCHW only.
// One thread per output element; used when the shape is not the AlignConv fast-path shape.
// mask / bias: the modulated form (DCNv2: modulated_deformable_im2col_gpu_kernel, deform_conv_cuda_kernel.cu:570-632:
// every sampled value is multiplied by mask[b, dg, tap, ho, wo]; bias added after the contraction,
// deform_conv_cuda.cpp:566-568); both null = plain deformable convolution.
// arithmetic type of the generic kernel: the reference instantiates its kernels per scalar type
// (AT_DISPATCH_FLOATING_TYPES_AND_HALF, deform_conv_cuda_kernel.cu:258,352,450): double stays double; float and half compute in
// float here (half columns rounded once, as the fused f16 path)
template <typename T>
struct GenAcc { using type = float; };
template <>
struct GenAcc<double> { using type = double; };

template <typename T, typename TO>
__global__ __launch_bounds__(256) void k_dcn_generic(const T* __restrict__ x, const TO* __restrict__ offset,
                                                     const T* __restrict__ w, T* __restrict__ out,
                                                     s2a_dcn_params p, int Ho, int Wo,
                                                     const T* __restrict__ mask = nullptr,
                                                     const T* __restrict__ bias = nullptr) {
  using A = typename GenAcc<T>::type;
  const int64_t total = p.batch * p.out_channels * Ho * Wo;
  const int Cg = (int)(p.channels / p.group), Og = (int)(p.out_channels / p.group);
  const int cpdg = (int)(p.channels / p.deformable_group);
  const int H = (int)p.height, W = (int)p.width;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    int wo = (int)(e % Wo);
    int64_t r = e / Wo;
    int ho = (int)(r % Ho);
    r /= Ho;
    int o = (int)(r % p.out_channels);
    int64_t b = r / p.out_channels;
    int g = o / Og;
    A acc = 0;
    for (int cl = 0; cl < Cg; cl++) {
      int c = g * Cg + cl;
      int dg = c / cpdg;
      const T* plane = x + (b * p.channels + c) * (int64_t)H * W;
      const TO* offp = offset + (b * p.deformable_group + dg) * 2 * p.kH * p.kW * (int64_t)Ho * Wo;
      const T* maskp = mask ? mask + (b * p.deformable_group + dg) * p.kH * p.kW * (int64_t)Ho * Wo : nullptr;
      for (int i = 0; i < p.kH; i++)
        for (int j = 0; j < p.kW; j++) {
          int t = i * p.kW + j;
          A oh = (A)offp[((int64_t)(2 * t) * Ho + ho) * Wo + wo];
          A ow = (A)offp[((int64_t)(2 * t + 1) * Ho + ho) * Wo + wo];
          A h_im = (A)(ho * p.dH - p.padH + i * p.dilationH) + oh;
          A w_im = (A)(wo * p.dW - p.padW + j * p.dilationW) + ow;
          A v = 0;
          if (h_im > -1 && w_im > -1 && h_im < H && w_im < W) {
            int h_low = (int)floor(h_im), w_low = (int)floor(w_im);
            int h_high = h_low + 1, w_high = w_low + 1;
            A lh = h_im - h_low, lw = w_im - w_low, hh = 1 - lh, hw = 1 - lw;
            A v1 = 0, v2 = 0, v3 = 0, v4 = 0;
            if (h_low >= 0 && w_low >= 0) v1 = (A)plane[h_low * W + w_low];
            if (h_low >= 0 && w_high <= W - 1) v2 = (A)plane[h_low * W + w_high];
            if (h_high <= H - 1 && w_low >= 0) v3 = (A)plane[h_high * W + w_low];
            if (h_high <= H - 1 && w_high <= W - 1) v4 = (A)plane[h_high * W + w_high];
            v = hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4;
          }
          if (maskp) v *= (A)maskp[((int64_t)t * Ho + ho) * Wo + wo];
          if (sizeof(T) == 2) v = (A)(T)v;  // f16 columns, as the f16 fast path
          acc += (A)w[(((int64_t)o * Cg + cl) * p.kH + i) * p.kW + j] * v;
        }
    }
    if (bias) acc += (A)bias[o];
    if (p.relu) acc = acc > 0 ? acc : (A)0;
    out[e] = (T)acc;
  }
}

inline bool fast_path_ok(const s2a_dcn_params& p) {
  if (p.dtype == S2A_DTYPE_F64) return false;       // float64: the generic kernel (API completeness, not a hot path)
  int kc = p.dtype == S2A_DTYPE_F32 ? 32 : 64;
  return p.kW == 3 && p.kH == 3 && p.dW == 1 && p.dH == 1 && p.padW == 1 && p.padH == 1 &&
         p.dilationW == 1 && p.dilationH == 1 && p.group == 1 && p.deformable_group == 1 &&
         p.channels % kc == 0 && p.out_channels % 64 == 0 && p.offset_dtype == S2A_DTYPE_F32 &&
         p.batch * p.height * p.width < (1ll << 31);
}

inline size_t esize(int dtype) { return dtype == S2A_DTYPE_F64 ? 8 : (dtype == S2A_DTYPE_F32 ? 4 : 2); }

inline bool half_coords_requested() {
  const char* f = getenv("S2A_DCN_HALF_COORDS");
  return f && atoi(f) != 0;
}

// position tiles of 16 x (npos / 16) positions
inline int64_t dcn_tiles(int64_t B, int H, int W, int npos) {
  return B * (int64_t)((W + 15) / 16) * ((H + npos / 16 - 1) / (npos / 16));
}

// the kernels' <OUT_NHWC, SRC> template arguments from the call's output layout and coordinate source
template <typename F>
int with_layout_src(bool out_nhwc, bool from_anchors, F&& launch) {
  using Anchors = std::integral_constant<int, 1>;
  using Offsets = std::integral_constant<int, 0>;
  if (out_nhwc) return from_anchors ? launch(std::true_type{}, Anchors{}) : launch(std::true_type{}, Offsets{});
  return from_anchors ? launch(std::false_type{}, Anchors{}) : launch(std::false_type{}, Offsets{});
}

template <typename T, bool NHWC, int SRC, int NPOS>
int launch_mfma(const T* x_nhwc, const float* src, const T* wp, T* out, int64_t B, int C, int H, int W, int O,
                float stride, int relu, hipStream_t st) {
  auto kern = k_dcn_mfma<T, NHWC, SRC, NPOS>;
  constexpr int lds = mfma_lds_bytes<NPOS>();
  dim3 grid((unsigned)dcn_tiles(B, H, W, NPOS), (unsigned)((O + kMaxO - 1) / kMaxO));
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  kern<<<grid, 256, lds, st>>>(x_nhwc, src, wp, out, B * (int64_t)H * W, C, H, W, O, stride, relu);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

// f32: the three-bf16-plane kernel (its filter planes sit behind the f32 stage layout in the packed buffer) unless
// S2A_DCN_F32=mfma32 asks for the f32 matrix instruction
int launch_fast(const float* x_nhwc, const float* src, bool from_anchors, const float* wp, float* out, bool out_nhwc,
                int64_t B, int C, int H, int W, int O, float stride, int relu, hipStream_t st) {
  // 128-position tiles once they still give every CU >= 2 workgroups; else 64
  const bool big = dcn_tiles(B, H, W, 128) >= 512;
  const char* sel = getenv("S2A_DCN_F32");
  const bool mfma32 = sel && sel[0] == 'm';
  const __bf16* wx3 = reinterpret_cast<const __bf16*>(wp + (size_t)O * C * 9);
  return with_layout_src(out_nhwc, from_anchors, [&](auto nhwc_c, auto src_c) {
    constexpr bool NHWC = decltype(nhwc_c)::value;
    constexpr int SRC = decltype(src_c)::value;
    auto x3 = [&](auto npos_c) {
      constexpr int NPOS = decltype(npos_c)::value;
      auto kern = k_dcn_x3<NHWC, SRC, NPOS>;
      constexpr int lds = x3_lds_bytes<NPOS>();
      dim3 grid((unsigned)dcn_tiles(B, H, W, NPOS), (unsigned)((O + kMaxO - 1) / kMaxO));
      S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      kern<<<grid, 512, lds, st>>>(x_nhwc, src, wx3, out, B * (int64_t)H * W, C, H, W, O, stride, relu);
      S2A_LAUNCH_CHECK();
      return S2A_OK;
    };
    if (mfma32)
      return big ? launch_mfma<float, NHWC, SRC, 128>(x_nhwc, src, wp, out, B, C, H, W, O, stride, relu, st)
                 : launch_mfma<float, NHWC, SRC, 64>(x_nhwc, src, wp, out, B, C, H, W, O, stride, relu, st);
    return big ? x3(std::integral_constant<int, 128>{}) : x3(std::integral_constant<int, 64>{});
  });
}

// f16: the patch-staged kernel; launches it cannot take (fewer than 128 tiles, a map side its 16-bit table coordinates cannot
// hold, an input beyond 32-bit byte offsets) run k_dcn_mfma on 64-position tiles
int launch_fast(const _Float16* x_nhwc, const float* src, bool from_anchors, const _Float16* wp, const _Float16* wfrag,
                _Float16* out, bool out_nhwc, int64_t B, int C, int H, int W, int O, float stride, int relu,
                hipStream_t st) {
  const int64_t Ntot = B * (int64_t)H * W;
  const int64_t tiles = dcn_tiles(B, H, W, 128);
  const uint64_t x_bytes = (uint64_t)Ntot * C * 2;
  const bool patch_ok = tiles >= 128 && x_bytes < (1ull << 31) && wfrag != nullptr && C % 64 == 0 && H < 32000 && W < 32000;
  // S2A_DCN_HALF_COORDS=1: sampling coordinates and weights rounded as the reference's Half instantiation rounds them
  // (f16 inputs only -- the f32 instantiation keeps f32 coordinates; built into the patch-staged kernel alone)
  const int hc_bit = half_coords_requested() ? 2 : 0;
  if (hc_bit && !patch_ok) {
    set_error("deform_conv: S2A_DCN_HALF_COORDS=1 needs the patch-staged f16 kernel (>= 128 position tiles, C %% 64 == 0)");
    return S2A_ENOTIMPL;
  }
  if (!patch_ok)
    return with_layout_src(out_nhwc, from_anchors, [&](auto nhwc_c, auto src_c) {
      return launch_mfma<_Float16, decltype(nhwc_c)::value, decltype(src_c)::value, 64>(x_nhwc, src, wp, out, B, C, H, W, O,
                                                                                        stride, relu, st);
    });
  // One 153 KB workgroup per CU: a launch whose 8 x 16 tiles fill the last round badly (one P3 level of ONE chip: 128
  // tiles on 256 CUs, BASELINE configs[1]) runs as 4 x 16 half tiles instead when that needs less time (bit-identical)
  int n_cu = 0;
  {
    int rc_ = device_cu_count(&n_cu);
    if (rc_ != S2A_OK) return rc_;
  }
  // rounds of one workgroup per CU; a half tile takes ~0.62 of a full one (measured: 128 tiles 44.5 -> 34.8 us as 256 half
  // tiles, but 256 tiles -- exactly one full round -- 50 -> 61 us as 512 half tiles)
  const int64_t rounds_full = (tiles + n_cu - 1) / n_cu, rounds_half = (2 * tiles + n_cu - 1) / n_cu;
  const bool half_tiles = 62 * rounds_half < 100 * rounds_full && !getenv("S2A_DCN_NO_HALF");
  const PatchArgs args{x_nhwc, src, wfrag, out, Ntot, C, H, W, O, stride, (relu ? 1 : 0) | hc_bit, (unsigned)x_bytes, 0, 0u, LevelTab{}};
  const unsigned ogroups = (unsigned)((O + kMaxO - 1) / kMaxO);
  return with_layout_src(out_nhwc, from_anchors, [&](auto nhwc_c, auto src_c) {
    constexpr bool NHWC = decltype(nhwc_c)::value;
    constexpr int SRC = decltype(src_c)::value;
    if (half_tiles) {
      constexpr int kHalfLds = 64 * 9 * 16 + 2 * 64 * kRowBytes + 2 * (4 + 2 * kHalo) * kPW * 128;
      auto kern = k_dcn_patch<NHWC, SRC, 4>;
      S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kHalfLds));
      kern<<<dim3((unsigned)(2 * tiles), ogroups), 512, kHalfLds, st>>>(args);
    } else {
      auto kern = k_dcn_patch<NHWC, SRC>;
      S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kPatchLds));
      kern<<<dim3((unsigned)tiles, ogroups), 512, kPatchLds, st>>>(args);
    }
    S2A_LAUNCH_CHECK();
    return S2A_OK;
  });
}

template <typename T>
int run_fast(const void* input, const float* src, bool from_anchors, const void* weight, void* output,
             int64_t B, int C, int H, int W, int O, int layout, float stride, int relu, void* ws,
             size_t ws_bytes, hipStream_t st, bool weight_packed = false) {
  constexpr int KC = Traits<T>::KC;
  S2A_CHECK_ARG(((uintptr_t)input % 16) == 0 && ((uintptr_t)output % 16) == 0 && ((uintptr_t)weight % 16) == 0 &&
                ((uintptr_t)ws % 16) == 0, "deform_conv: tensors must be 16-byte aligned");
  Carver cv(ws, ws_bytes);
  const size_t wel = (size_t)O * C * 9;
  const bool has_frag = sizeof(T) == 2;             // f16 packs both layouts back to back; f32: the stage layout, then the three bf16 planes
  T* wp = weight_packed ? const_cast<T*>((const T*)weight) : cv.take<T>(has_frag ? wel * 2 : wel * 5 / 2);
  T* xn = nullptr;
  if (layout == S2A_LAYOUT_NCHW) xn = cv.take<T>((size_t)B * C * H * W);
  if (!wp || (layout == S2A_LAYOUT_NCHW && !xn)) {
    set_error("deform_conv: workspace too small (%zu < %zu)", ws_bytes, cv.off);
    return S2A_EWORKSPACE;
  }
  const int64_t wtot = (int64_t)O * C * 9;
  if (!weight_packed) {
    k_pack_weight<T><<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const T*)weight, O, C, KC, wp);
    if constexpr (sizeof(T) == 2) {
      k_pack_weight_frag16<<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const _Float16*)weight, O, C, wp + wel);
    } else {
      k_pack_weight_x3<<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const float*)weight, O, C, reinterpret_cast<__bf16*>(wp + wel));
    }
  }
  const T* x_nhwc = (const T*)input;
  if (layout == S2A_LAYOUT_NCHW) {
    int64_t HW = (int64_t)H * W;
    dim3 g((unsigned)((HW + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
    k_nchw_to_nhwc<T><<<g, 256, 0, st>>>((const T*)input, B, C, HW, xn);
    x_nhwc = xn;
  }
  if constexpr (sizeof(T) == 2)
    return launch_fast(x_nhwc, src, from_anchors, wp, wp + wel, (T*)output, layout == S2A_LAYOUT_NHWC, B, C, H, W, O, stride,
                       relu, st);
  else
    return launch_fast(x_nhwc, src, from_anchors, wp, (T*)output, layout == S2A_LAYOUT_NHWC, B, C, H, W, O, stride, relu, st);
}

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" size_t s2a_deform_conv_workspace_bytes(const s2a_dcn_params* p) {
  if (!p || p->batch < 0 || p->channels <= 0 || p->out_channels <= 0 || p->height <= 0 || p->width <= 0 || p->kH <= 0 || p->kW <= 0 ||
      (p->dtype != S2A_DTYPE_F32 && p->dtype != S2A_DTYPE_F16 && p->dtype != S2A_DTYPE_F64))
    return 0;   // (parameters the entry point refuses)
  size_t es = esize(p->dtype);
  size_t b = align_up((size_t)p->out_channels * p->channels * p->kH * p->kW * es * 3) + 256;      // a BOUND for the fast and the generic path, not the image of a carve (packed filter: f16 two layouts, f32 2.5 x)
  if (p->layout == S2A_LAYOUT_NCHW) b += align_up((size_t)p->batch * p->channels * p->height * p->width * es);
  return b;
}

extern "C" int s2a_deform_conv_forward(const void* input, const void* weight, const void* offset,
                                       void* output, const s2a_dcn_params* pp, void* workspace,
                                       size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(pp != nullptr, "deform_conv: NULL params");
  const s2a_dcn_params p = *pp;
  // shape_check (deform_conv_cuda.cpp:62-150)
  S2A_CHECK_ARG(p.kW > 0 && p.kH > 0, "kernel size should be greater than zero, but got kH: %d kW: %d", p.kH, p.kW);
  S2A_CHECK_ARG(p.dW > 0 && p.dH > 0, "stride should be greater than zero, but got dH: %d dW: %d", p.dH, p.dW);
  S2A_CHECK_ARG(p.dilationW > 0 && p.dilationH > 0, "dilation should be greater than 0, but got dilationH: %d dilationW: %d", p.dilationH, p.dilationW);
  S2A_CHECK_ARG(p.group > 0 && p.deformable_group > 0, "deform_conv: group counts must be positive");
  S2A_CHECK_ARG(p.channels % p.group == 0 && p.out_channels % p.group == 0, "deform_conv: channels must divide groups");
  S2A_CHECK_ARG(p.channels % p.deformable_group == 0, "input channels must divide deformable group size");
  S2A_CHECK_ARG(p.dtype == S2A_DTYPE_F32 || p.dtype == S2A_DTYPE_F16 || p.dtype == S2A_DTYPE_F64, "deform_conv: dtype");
  S2A_CHECK_ARG(p.dtype == S2A_DTYPE_F64 ? p.offset_dtype == S2A_DTYPE_F64 : (p.offset_dtype == S2A_DTYPE_F32 || p.offset_dtype == p.dtype),
                "deform_conv: offset dtype (float64 input: float64 offsets; otherwise float32 or the input's)");
  const int64_t Ho = (p.height + 2 * p.padH - (p.dilationH * (p.kH - 1) + 1)) / p.dH + 1;
  const int64_t Wo = (p.width + 2 * p.padW - (p.dilationW * (p.kW - 1) + 1)) / p.dW + 1;
  S2A_CHECK_ARG(Ho >= 1 && Wo >= 1, "Given input size: (%lld x %lld x %lld). Calculated output size: (%lld x %lld x %lld). Output size is too small",
                (long long)p.channels, (long long)p.height, (long long)p.width, (long long)p.out_channels, (long long)Ho, (long long)Wo);
  S2A_CHECK_ARG(p.height >= p.kH && p.width >= p.kW, "input image is smaller than kernel");
  if (p.batch == 0) return S2A_OK;
  S2A_CHECK_ARG(input && weight && offset && output, "deform_conv: NULL tensor");
  // (one rule for both paths: the generic kernel needs no scratch, a caller of the header does not know which path runs)
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_deform_conv_workspace_bytes(pp), "deform_conv_forward");
  hipStream_t st = as_stream(stream);
  if (fast_path_ok(p)) {
    if (p.dtype == S2A_DTYPE_F32)
      return run_fast<float>(input, (const float*)offset, false, weight, output, p.batch, (int)p.channels,
                             (int)p.height, (int)p.width, (int)p.out_channels, p.layout, 1.f, p.relu,
                             workspace, workspace_bytes, st);
    return run_fast<_Float16>(input, (const float*)offset, false, weight, output, p.batch, (int)p.channels,
                              (int)p.height, (int)p.width, (int)p.out_channels, p.layout, 1.f, p.relu,
                              workspace, workspace_bytes, st);
  }
  S2A_CHECK_ARG(p.layout == S2A_LAYOUT_NCHW, "deform_conv: the generic path supports NCHW only");
  const int64_t total = p.batch * p.out_channels * Ho * Wo;
  unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 65535);
  if (p.dtype == S2A_DTYPE_F64)
    k_dcn_generic<double, double><<<g, 256, 0, st>>>((const double*)input, (const double*)offset, (const double*)weight, (double*)output, p, (int)Ho, (int)Wo);
  else if (p.dtype == S2A_DTYPE_F32)
    k_dcn_generic<float, float><<<g, 256, 0, st>>>((const float*)input, (const float*)offset, (const float*)weight, (float*)output, p, (int)Ho, (int)Wo);
  else if (p.offset_dtype == S2A_DTYPE_F32)
    k_dcn_generic<_Float16, float><<<g, 256, 0, st>>>((const _Float16*)input, (const float*)offset, (const _Float16*)weight, (_Float16*)output, p, (int)Ho, (int)Wo);
  else
    k_dcn_generic<_Float16, _Float16><<<g, 256, 0, st>>>((const _Float16*)input, (const _Float16*)offset, (const _Float16*)weight, (_Float16*)output, p, (int)Ho, (int)Wo);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_modulated_deform_conv_forward(const void* input, const void* weight, const void* bias,
                                                 const void* offset, const void* mask, void* output,
                                                 const s2a_dcn_params* pp, s2a_stream_t stream) {
  S2A_CHECK_ARG(pp != nullptr, "modulated_deform_conv: NULL params");
  const s2a_dcn_params p = *pp;
  S2A_CHECK_ARG(p.kW > 0 && p.kH > 0 && p.dW > 0 && p.dH > 0 && p.dilationW > 0 && p.dilationH > 0,
                "modulated_deform_conv: kernel size, stride and dilation must be positive");
  S2A_CHECK_ARG(p.group > 0 && p.deformable_group > 0 && p.channels % p.group == 0 && p.out_channels % p.group == 0 &&
                p.channels % p.deformable_group == 0, "Input shape and kernel channels wont match");
  S2A_CHECK_ARG(p.dtype == S2A_DTYPE_F32 || p.dtype == S2A_DTYPE_F16, "modulated_deform_conv: dtype");
  S2A_CHECK_ARG(p.offset_dtype == p.dtype, "modulated_deform_conv: offset and mask share the input dtype");
  S2A_CHECK_ARG(p.layout == S2A_LAYOUT_NCHW, "modulated_deform_conv: NCHW only");
  const int64_t Ho = (p.height + 2 * p.padH - (p.dilationH * (p.kH - 1) + 1)) / p.dH + 1;
  const int64_t Wo = (p.width + 2 * p.padW - (p.dilationW * (p.kW - 1) + 1)) / p.dW + 1;
  S2A_CHECK_ARG(Ho >= 1 && Wo >= 1, "modulated_deform_conv: output size is too small");
  if (p.batch == 0) return S2A_OK;
  S2A_CHECK_ARG(input && weight && offset && mask && output, "modulated_deform_conv: NULL tensor");
  hipStream_t st = as_stream(stream);
  const int64_t total = p.batch * p.out_channels * Ho * Wo;
  unsigned g = (unsigned)std::min<int64_t>((total + 255) / 256, 65535);
  if (p.dtype == S2A_DTYPE_F32)
    k_dcn_generic<float, float><<<g, 256, 0, st>>>((const float*)input, (const float*)offset, (const float*)weight,
                                                   (float*)output, p, (int)Ho, (int)Wo, (const float*)mask, (const float*)bias);
  else
    k_dcn_generic<_Float16, _Float16><<<g, 256, 0, st>>>((const _Float16*)input, (const _Float16*)offset, (const _Float16*)weight,
                                                         (_Float16*)output, p, (int)Ho, (int)Wo, (const _Float16*)mask,
                                                         (const _Float16*)bias);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" size_t s2a_align_conv_workspace_bytes(const s2a_align_params* p) {
  if (!p || p->batch < 0 || p->channels <= 0 || p->out_channels <= 0 || p->height < 3 || p->width < 3 ||
      (p->dtype != S2A_DTYPE_F32 && p->dtype != S2A_DTYPE_F16))
    return 0;   // (parameters the entry point refuses)
  size_t es = esize(p->dtype);
  size_t b = align_up((size_t)p->out_channels * p->channels * 9 * es * 3) + 256;      // a BOUND for the fast and the generic path, not the image of a carve (packed filter: f16 two layouts, f32 2.5 x)
  if (p->layout == S2A_LAYOUT_NCHW) b += align_up((size_t)p->batch * p->channels * p->height * p->width * es);
  return b;
}

extern "C" int s2a_align_conv_forward(const void* x, const float* anchors, const void* weight, void* out,
                                      const s2a_align_params* pp, void* workspace,
                                      size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(pp != nullptr, "align_conv: NULL params");
  const s2a_align_params p = *pp;
  S2A_CHECK_ARG(p.dtype == S2A_DTYPE_F32 || p.dtype == S2A_DTYPE_F16, "align_conv: dtype");
  S2A_CHECK_ARG(p.stride > 0, "align_conv: stride must be positive");
  const int kc = p.dtype == S2A_DTYPE_F32 ? 32 : 64;
  S2A_CHECK_ARG(p.channels % kc == 0 && p.out_channels % 64 == 0,
                "align_conv: channels must be a multiple of %d and out_channels of 64", kc);
  S2A_CHECK_ARG(p.height >= 3 && p.width >= 3, "input image is smaller than kernel");
  S2A_CHECK_ARG(p.batch * p.height * p.width < (1ll << 31), "align_conv: too many positions");
  if (p.batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && anchors && weight && out, "align_conv: NULL tensor");
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_align_conv_workspace_bytes(pp), "align_conv_forward");
  hipStream_t st = as_stream(stream);
  if (p.dtype == S2A_DTYPE_F32)
    return run_fast<float>(x, anchors, true, weight, out, p.batch, (int)p.channels, (int)p.height,
                           (int)p.width, (int)p.out_channels, p.layout, p.stride, p.relu, workspace,
                           workspace_bytes, st, p.weight_packed != 0);
  return run_fast<_Float16>(x, anchors, true, weight, out, p.batch, (int)p.channels, (int)p.height,
                            (int)p.width, (int)p.out_channels, p.layout, p.stride, p.relu, workspace,
                            workspace_bytes, st, p.weight_packed != 0);
}

extern "C" int s2a_dcn_pack_weight(const void* weight, int64_t out_channels, int64_t channels,
                                   int dtype, void* packed, s2a_stream_t stream) {
  S2A_CHECK_ARG(dtype == S2A_DTYPE_F32 || dtype == S2A_DTYPE_F16, "dcn_pack_weight: dtype");
  const int kc = dtype == S2A_DTYPE_F32 ? 32 : 64;
  S2A_CHECK_ARG(out_channels > 0 && channels > 0 && channels % kc == 0,
                "dcn_pack_weight: channels must be a multiple of %d", kc);
  S2A_CHECK_ARG(weight && packed, "dcn_pack_weight: NULL tensor");
  const int64_t wtot = out_channels * channels * 9;
  hipStream_t st = as_stream(stream);
  if (dtype == S2A_DTYPE_F32) {
    k_pack_weight<float><<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const float*)weight, (int)out_channels, (int)channels, kc, (float*)packed);
    k_pack_weight_x3<<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const float*)weight, (int)out_channels, (int)channels,
                                                                    reinterpret_cast<__bf16*>((float*)packed + wtot));
  } else {
    S2A_CHECK_ARG(out_channels % 64 == 0, "dcn_pack_weight: out_channels must be a multiple of 64");
    k_pack_weight<_Float16><<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const _Float16*)weight, (int)out_channels, (int)channels, kc, (_Float16*)packed);
    k_pack_weight_frag16<<<(unsigned)((wtot + 255) / 256), 256, 0, st>>>((const _Float16*)weight, (int)out_channels, (int)channels, (_Float16*)packed + wtot);
  }
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int64_t s2a_dcn_packed_elems(int64_t out_channels, int64_t channels, int dtype) {
  // f16 holds two layouts back to back (stage-major for the LDS-staged kernels, MFMA-fragment order for the patch-staged kernel);
  // f32: the stage-major f32 layout, then the filter's three bf16 planes (k_dcn_x3): 1 + 1.5 elements per weight
  const int64_t wel = out_channels * channels * 9;
  return dtype == S2A_DTYPE_F16 ? wel * 2 : wel * 5 / 2;
}

namespace s2a {
int build_flags_dcn() {
  int f = 0;
  if (S2A_STAMP) f |= 1 << 9;
#ifdef S2A_MEASURE
  f |= 1 << 10;
#endif
  return f;
}
}  // namespace s2a

extern "C" int s2a_debug_read_stamps(unsigned long long* host_dst, int64_t count) {
#if S2A_STAMP
  S2A_HIP(hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(s2a::g_stamps), (size_t)count * 8));
  return S2A_OK;
#else
  (void)host_dst; (void)count;
  s2a::set_error("s2a_debug_read_stamps: not a diagnostic build");
  return S2A_ENOTIMPL;
#endif
}

extern "C" int s2a_align_conv_pyramid_f16(const void* x, const float* anchors, const void* weight_packed, void* out,
                                          int64_t batch, int64_t channels, int64_t out_channels, int relu,
                                          const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0, "align_conv_pyramid: bad shape");
  S2A_CHECK_ARG(channels % 64 == 0 && out_channels % 64 == 0, "align_conv_pyramid: channels and out_channels must be multiples of 64");
  LevelTab lt; int64_t pix = 0;
  const int64_t tiles = build_levels(pyr, batch, &lt, &pix);
  S2A_CHECK_ARG(tiles >= 0, "align_conv_pyramid: bad level table (1..8 levels, positive sizes)");
  for (int i = 0; i < lt.n; i++) {
    S2A_CHECK_ARG(lt.stride[i] > 0, "align_conv: stride must be positive");
    S2A_CHECK_ARG(lt.H[i] >= 3 && lt.W[i] >= 3, "input image is smaller than kernel");
  }
  S2A_CHECK_ARG((uint64_t)pix * channels * 2 < (1ull << 31), "align_conv_pyramid: input too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && anchors && weight_packed && out, "align_conv_pyramid: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_packed % 16) == 0,
                "align_conv_pyramid: tensors must be 16-byte aligned");
  if (lt.n == 1) lt.n = 2, lt.tile0[1] = 0x7fffffff;
  hipStream_t st = as_stream(stream);
  // s2a_dcn_pack_weight (f16) = stage-major layout followed by the MFMA-fragment layout
  const _Float16* wfrag = (const _Float16*)weight_packed + (size_t)out_channels * channels * 9;
  // (Forms of this launch that were built, tested bit-identical, measured on MI355X and removed again -- DESIGN.md 4 has the
  // numbers: a persistent workgroup per CU with the next tile's anchors / patch prefetched (245 vs 232 us: spills), a
  // three-slot column ring with loaders two stages ahead (2-8 % slower), two half-tile workgroups per CU (332 vs 282 us:
  // the filter streamed twice), half tiles for the last round in a second launch (-1.2 %).)
  const unsigned ogroups = (unsigned)((out_channels + kMaxO - 1) / kMaxO);
  const int relu_flags = (relu ? 1 : 0) | (half_coords_requested() ? 2 : 0);
  auto kern = k_dcn_patch<true, 1>;
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kPatchLds));
  // the last round as half tiles when it would leave more than half of the CUs idle (see k_dcn_patch); S2A_DCN_HALF_TAIL=0|1 forces
  int ncu = 0;
  {
    int rc_ = device_cu_count(&ncu);
    if (rc_ != S2A_OK) return rc_;
  }
  const int64_t rem = tiles % ncu;
  bool half_tail = tiles > ncu && rem != 0 && 2 * rem <= ncu;
  if (const char* f = getenv("S2A_DCN_HALF_TAIL")) half_tail = atoi(f) != 0 && tiles > rem && rem != 0;
  const unsigned n_full = half_tail ? (unsigned)(tiles - rem) : 0u;
  const unsigned grid_x = half_tail ? (unsigned)(tiles - rem + 2 * rem) : (unsigned)tiles;
  kern<<<dim3(grid_x, ogroups), 512, kPatchLds, st>>>(PatchArgs{(const _Float16*)x, anchors, wfrag, (_Float16*)out, 0, (int)channels,
                                                      lt.H[0], lt.W[0], (int)out_channels, lt.stride[0], relu_flags, 0u, 0, n_full, lt});
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
