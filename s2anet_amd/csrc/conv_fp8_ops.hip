// FP8 (OCP e4m3fn) 3x3 convolution for the head towers on MI355X (gfx950), on the block-scaled matrix instruction
// v_mfma_scale_f32_16x16x128_f8f6f4 with every block scale 1.0: 4x the K of v_mfma_f32_16x16x32_f16 in 2x the cycles, and
// half the operand bytes in HBM, in the LDS patch and per ds_read.
//
// k_quantize_e4m3 (f16 rows -> e4m3 bytes), k_pack_weight_fp8 (e4m3 filter -> fragment order) and k_conv3x3_fp8, which is
// k_conv_f16<9, 4> (conv_ops.hip) restated for one-byte operands: the same 8 x 16-position x 256-channel tile, the patch by
// LDS-DMA at the same 144-byte pixel pitch (128 channels of e4m3 where the f16 kernel holds 64 halfs), the filter in
// fragment order from L2 one stage ahead in registers, the epilogue staged through LDS and stored as whole rows.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "mfma_common.hpp"

namespace s2a {
namespace {

using i32x8 = __attribute__((ext_vector_type(8))) int;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x2 = __attribute__((ext_vector_type(2))) int;

// two f32 -> two e4m3 bytes (round to nearest even, subnormals kept) in the low half of the result.  The inputs are
// clamped to +-448 by the callers, so the conversion never meets its overflow rule; NaN stays NaN.
__device__ __forceinline__ unsigned cvt2_e4m3(float a, float b) {
  return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}
// clamp that keeps NaN (fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp448(float v) {
  return v != v ? v : __builtin_fminf(__builtin_fmaxf(v, -448.f), 448.f);
}

// ------------------------------------------------------------------ quantise
// x [n8 * 8] f16 -> q [n8 * 8] e4m3: q = e4m3_rne(clamp(f32(x) * inv_scale, -448, 448)); 16 B in, 8 B out per lane.
// +-inf saturate (the clamp), NaN -> the e4m3 NaN of the same sign (0x7f | sign: the only NaN encoding of e4m3fn).
__global__ __launch_bounds__(256) void k_quantize_e4m3(const f16x8* __restrict__ x, i32x2* __restrict__ q, int64_t n8,
                                                       float inv_scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const f16x8 v = x[i];
  unsigned w[2] = {0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const float a = (float)v[e] * inv_scale, b = (float)v[e + 1] * inv_scale;
    unsigned p = cvt2_e4m3(clamp448(a), clamp448(b));
    if (a != a) p = (p & 0xff00u) | 0x7fu | ((__float_as_uint(a) >> 24) & 0x80u);
    if (b != b) p = (p & 0x00ffu) | 0x7f00u | ((__float_as_uint(b) >> 16) & 0x8000u);
    w[e >> 2] |= p << (16 * ((e >> 1) & 1));
  }
  q[i] = i32x2{(int)w[0], (int)w[1]};
}

// ------------------------------------------------------------------ filter pack
// 16x16x128 operand maps (established with exact integer data on the chip): lane l = (i = l & 15, kg = l >> 4)
// holds row i of A (column i of B) and 32 of the 128 k-values in its 32 operand bytes; byte j of lane group kg is the same
// k for A and B, so any assignment of channels to (kg, j) is valid as long as filter and patch agree.  Here the two 16-byte
// halves h of lane group kg are the 16-channel runs c(kg, h) = {0, 4, 1, 5}[kg] + 2 h of the 128-channel chunk: the 16-byte
// slots k_conv_f16 reads at these lanes, conflict-free at the 144-byte pixel pitch with its pixel map.
//
// weight [O][C][9] e4m3 -> [stage = cc*9 + t][och group of 64][m-tile a 4][half h 2][lane 64][16 bytes]:
// byte j = W[g*64 + a*16 + (l & 15)][cc*128 + 16 c(l >> 4, h) + j][t]
__device__ __forceinline__ int chan_run(int kg, int h) { return (kg & 1) * 4 + (kg >> 1) + 2 * h; }

__global__ void k_pack_weight_fp8(const uint8_t* __restrict__ w, int O, int C, uint8_t* __restrict__ wp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)O * C * 9) return;
  const int G = O / 64;
  const int j = (int)(e & 15), lane = (int)((e >> 4) & 63), h = (int)((e >> 10) & 1), a = (int)((e >> 11) & 3);
  const int64_t r = e >> 13;
  const int g = (int)(r % G), st = (int)(r / G);
  const int t = st % 9, cc = st / 9;
  const int och = g * 64 + a * 16 + (lane & 15);
  const int k = cc * 128 + 16 * chan_run(lane >> 4, h) + j;
  wp[e] = w[((int64_t)och * C + k) * 9 + t];
}

// ------------------------------------------------------------------ 3x3 / stride 1 / pad 1, e4m3 operands
constexpr int kPW = 18;                                   // patch width: 16 positions + 1 halo each side
constexpr int kTH = 8, kPos = 128;                        // tile rows, positions per workgroup
constexpr int kPix = (kTH + 2) * kPW;                     // 180 patch pixels
constexpr int kDma = (kPix * 9 + 63) / 64;                // 1 KB LDS-DMA pieces per patch (26)
constexpr int kPatchBytes = kDma * 1024;
constexpr int kJ = (kDma + 3) / 4;                        // DMA pieces per wave
constexpr int kRowF16 = 4 * 128 + 16, kRowF8 = 256 + 16;  // staged output rows (bytes)
constexpr int kLdsTile = (2 * kPatchBytes > kPos * kRowF16) ? 2 * kPatchBytes : kPos * kRowF16;
constexpr int kLdsFp8 = kLdsTile + 2048;                  // + scale[256], bias[256] f32

// acc[o] = sum x_q w_q (f32), v = acc * scale[o] + bias[o] (one fma), optional ReLU (NaN -> 0);
// OUT8 = false: out[P,O] f16;  OUT8 = true: out[P,O] e4m3 = e4m3_rne(clamp(v * out_inv_scale, +-448))
template <bool OUT8>
__global__ __launch_bounds__(256, 2) void k_conv3x3_fp8(const uint8_t* __restrict__ x, const uint8_t* __restrict__ wfrag,
                                                        const float* __restrict__ scale, const float* __restrict__ bias,
                                                        void* __restrict__ out_, int C, int O, int relu, float out_inv_scale,
                                                        LevelTab lt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t tile = xcd_remap(blockIdx.x, gridDim.x);
  int H = lt.H[0], W = lt.W[0];
  {                                     // this workgroup's level
    int t0 = 0, p0 = 0;
#pragma unroll
    for (int i = 0; i < kMaxLevels; i++)
      if (i < lt.n && tile >= lt.tile0[i]) {
        t0 = lt.tile0[i]; p0 = lt.pix0[i]; H = lt.H[i]; W = lt.W[i];
      }
    tile -= t0;
    x += (int64_t)p0 * C;
    out_ = reinterpret_cast<char*>(out_) + (int64_t)p0 * O * (OUT8 ? 1 : 2);
  }
  const int64_t Ntot = (int64_t)lt.batch * H * W, HW = (int64_t)H * W;
  const unsigned x_bytes = (unsigned)(Ntot * C);
  const int txn = (W + 15) / 16, tyn = (H + kTH - 1) / kTH;
  const int64_t bimg = tile / (txn * tyn);
  const int trem = (int)(tile % (txn * tyn));
  const int ty0 = (trem / txn) * kTH, tx0 = (trem % txn) * 16;
  const int o0 = blockIdx.y * 256;
  const int Oloc = min(256, O - o0);
  const int CC = C / 128, G = O / 64;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(x), 0, (int)x_bytes, 0x00020000);

  // patch: global -> LDS by LDS-DMA, linear slot v = pixel * 9 + 16-byte chunk (k_conv_f16's layout); the pad chunk and
  // pixels outside the image read an out-of-range offset (-> zero bytes = e4m3 +0)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  unsigned pvoff[kJ];
#pragma unroll
  for (int j = 0; j < kJ; j++) {
    const int v = (wave_u + 4 * j) * 64 + lane, p = v / 9, q = v % 9;
    const int yy = ty0 - 1 + p / kPW, xx = tx0 - 1 + p % kPW;
    const bool in = q < 8 && p < kPix && yy >= 0 && yy < H && xx >= 0 && xx < W;
    const int64_t pix = bimg * HW + (int64_t)yy * W + xx;
    pvoff[j] = in ? (unsigned)(pix * C + q * 16) : 0x80000000u;
  }
  auto patch_issue = [&](int cc) {
    char* P = smem + (cc & 1) * kPatchBytes;
#pragma unroll
    for (int j = 0; j < kJ; j++) {
      const int i = wave_u + 4 * j;
      if (i < kDma)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(P + i * 1024), 16,
                                                 (int)pvoff[j], cc * 128, 0, 0);
    }
  };
  float* s_scale = reinterpret_cast<float*>(smem + kLdsTile);
  float* s_bias = s_scale + 256;
  float scale_v = 0.f, bias_v = 0.f;
  if (tid < Oloc) { scale_v = scale[o0 + tid]; bias_v = bias[o0 + tid]; }

  const int grp = wave;                                   // wave = 64 out channels x the 128 positions
  const bool wave_active = grp * 64 < Oloc;
  const int g = min(o0 / 64 + grp, G - 1);
  i32x4 wA[4][2], wB[4][2];
  auto load_w = [&](int s, i32x4 (&wv)[4][2]) {
    const i32x4* p = reinterpret_cast<const i32x4*>(wfrag) + ((int64_t)s * G + g) * 512 + lane;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int h = 0; h < 2; h++) wv[a][h] = p[(a * 2 + h) * 64];
  };
  // lane -> (pixel, channel runs): k_conv_f16's 16x16 maps
  const int kg16 = lane >> 4, i16 = lane & 15;
  const int pix16 = (i16 >= 4 && i16 < 12) ? (((i16 - 4) >> 1) * 4 + (i16 & 1))
                                           : (((i16 & 3) >> 1) * 4 + 2 + (i16 & 1) + (i16 >= 12 ? 8 : 0));
  const int fbase16 = pix16 * kRowBytes + (kg16 & 1) * 64 + (kg16 >> 1) * 16;
  constexpr int kTile16 = kPW * kRowBytes;                // a wave's 16-position tiles are the tile's rows

  f32x4 acc[4][8];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 8; b++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[a][b][r] = 0.f;

  constexpr int kOne = 0x7f7f7f7f;                        // E8M0 block scales: 2^0
  auto compute = [&](const char* P, int t, const i32x4 (&wv)[4][2]) {
    if (!wave_active) return;
    const int toff = ((t / 3) * kPW + (t % 3)) * kRowBytes;
    i32x8 wf[4];
#pragma unroll
    for (int a = 0; a < 4; a++) wf[a] = __builtin_shufflevector(wv[a][0], wv[a][1], 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int bh = 0; bh < 8; bh += 4) {                   // four position tiles at a time (registers)
      i32x8 pf[4];
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const char* q = P + fbase16 + (bh + b) * kTile16 + toff;
        pf[b] = __builtin_shufflevector(*reinterpret_cast<const i32x4*>(q), *reinterpret_cast<const i32x4*>(q + 32), 0, 1, 2, 3,
                                        4, 5, 6, 7);
      }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
          acc[a][bh + b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[a], pf[b], acc[a][bh + b], 0, 0, 0, kOne, 0, kOne);
    }
  };

  const int last = 9 * CC - 1;
  patch_issue(0);
  load_w(0, wA);
  if (tid < 256) { s_scale[tid] = scale_v; s_bias[tid] = bias_v; }
  __syncthreads();   // (the DMA is drained with vmcnt(0) before the barrier)
  for (int cc = 0; cc < CC; cc++) {
    const int s0 = cc * 9;
    const char* Pc = smem + (cc & 1) * kPatchBytes;
#define S2A_TAP(T_, WCUR, WNEXT)                        \
    load_w(min(s0 + (T_) + 1, last), WNEXT);            \
    compute(Pc, (T_), WCUR);                            \
    __builtin_amdgcn_sched_barrier(0);
    S2A_TAP(0, wA, wB)
    S2A_TAP(1, wB, wA)
    S2A_TAP(2, wA, wB)
    S2A_TAP(3, wB, wA)
    S2A_TAP(4, wA, wB)
    S2A_TAP(5, wB, wA)
    if (cc + 1 < CC) patch_issue(cc + 1);                 // taps 6-8 cover its latency
    S2A_TAP(6, wA, wB)
    S2A_TAP(7, wB, wA)
    S2A_TAP(8, wA, wB)
#undef S2A_TAP
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int h = 0; h < 2; h++) wA[a][h] = wB[a][h];
  }

  // ---- epilogue: scale, bias, ReLU; tile staged through LDS (every wave is past the loop's last barrier), whole rows stored
  char* s_out = smem;
  constexpr int kRowB = OUT8 ? kRowF8 : kRowF16;
  using h4e = __attribute__((ext_vector_type(4))) _Float16;
  const bool relu_u = __builtin_amdgcn_readfirstlane(relu) != 0;
  if (wave_active) {
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int och = grp * 64 + 16 * a + 4 * kg16;       // D: row (out channel) = 4 (lane >> 4) + register, column = pixel
      const f32x4 sq = *reinterpret_cast<const f32x4*>(s_scale + och);
      const f32x4 bq = *reinterpret_cast<const f32x4*>(s_bias + och);
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const int pos = 16 * b + pix16;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          v[r] = __builtin_fmaf(acc[a][b][r], sq[r], bq[r]);
          if (relu_u) v[r] = __builtin_fmaxf(v[r], 0.f);
        }
        if constexpr (OUT8) {
#pragma unroll
          for (int r = 0; r < 4; r++) v[r] = clamp448(v[r] * out_inv_scale);
          *reinterpret_cast<unsigned*>(s_out + pos * kRowB + och) = cvt2_e4m3(v[0], v[1]) | (cvt2_e4m3(v[2], v[3]) << 16);
        } else {
          *reinterpret_cast<h4e*>(s_out + pos * kRowB + och * 2) = h4e{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        }
      }
    }
  }
  __syncthreads();
  constexpr int VPR = OUT8 ? 16 : 32;                     // 16-byte vectors per 256-channel row
  constexpr int EPV = OUT8 ? 16 : 8;                      // channels per vector
#pragma unroll
  for (int i = 0; i < kPos * VPR / 256; i++) {
    const int idx = tid + 256 * i, pos = idx / VPR, col = idx % VPR;
    const int64_t gp = tile_pos(tile, pos, kTH, H, W, HW, Ntot);
    if (gp >= 0 && col * EPV < Oloc)
      *reinterpret_cast<i32x4*>(reinterpret_cast<char*>(out_) + (gp * O + o0 + col * EPV) * (OUT8 ? 1 : 2)) =
          *reinterpret_cast<const i32x4*>(s_out + pos * kRowB + col * 16);
  }
}

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" int s2a_quantize_e4m3(const void* x, void* q, int64_t rows, int64_t channels, float inv_scale,
                                 s2a_stream_t stream) {
  S2A_CHECK_ARG(rows >= 0 && channels > 0, "quantize_e4m3: bad shape");
  S2A_CHECK_ARG(channels % 16 == 0, "quantize_e4m3: channels must be a multiple of 16");
  S2A_CHECK_ARG(x && q, "quantize_e4m3: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)q % 8) == 0, "quantize_e4m3: x must be 16-byte, q 8-byte aligned");
  const int64_t n8 = rows * channels / 8;
  S2A_CHECK_ARG((n8 + 255) / 256 < (1ll << 31), "quantize_e4m3: tensor too large");
  if (n8 == 0) return S2A_OK;
  k_quantize_e4m3<<<(unsigned)((n8 + 255) / 256), 256, 0, as_stream(stream)>>>((const f16x8*)x, (i32x2*)q, n8, inv_scale);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_conv_pack_weight_fp8(const void* weight_q, int64_t out_channels, int64_t channels, void* packed,
                                        s2a_stream_t stream) {
  S2A_CHECK_ARG(out_channels > 0 && channels > 0 && out_channels % 64 == 0 && channels % 128 == 0,
                "conv_pack_weight_fp8: out_channels must be a multiple of 64, channels a multiple of 128");
  S2A_CHECK_ARG(weight_q && packed, "conv_pack_weight_fp8: NULL tensor");
  const int64_t wtot = out_channels * channels * 9;
  S2A_CHECK_ARG(wtot < (1ll << 31), "conv_pack_weight_fp8: filter too large");
  k_pack_weight_fp8<<<(unsigned)((wtot + 255) / 256), 256, 0, as_stream(stream)>>>((const uint8_t*)weight_q, (int)out_channels,
                                                                                 (int)channels, (uint8_t*)packed);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_conv3x3_pyramid_fp8(const void* x_q, const void* weight_frag, const float* scale, const float* bias,
                                       void* out, int out_e4m3, float out_inv_scale, int64_t batch, int64_t channels,
                                       int64_t out_channels, int relu, const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0, "conv_pyramid_fp8: bad shape");
  S2A_CHECK_ARG(channels % 128 == 0 && out_channels % 64 == 0,
                "conv_pyramid_fp8: channels must be a multiple of 128, out_channels a multiple of 64");
  S2A_CHECK_ARG(x_q && weight_frag && scale && bias && out, "conv_pyramid_fp8: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x_q % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)scale % 4) == 0 && ((uintptr_t)bias % 4) == 0, "conv_pyramid_fp8: tensors must be 16-byte aligned");
  LevelTab lt; int64_t pix = 0;
  const int64_t tiles = build_levels(pyr, batch, &lt, &pix, kTH);
  S2A_CHECK_ARG(tiles >= 0, "conv_pyramid_fp8: bad level table (1..8 levels, positive sizes)");
  S2A_CHECK_ARG((uint64_t)pix * channels < (1ull << 31), "conv_pyramid_fp8: input too large for 32-bit offsets");
  if (batch == 0 || tiles == 0) return S2A_OK;
  const dim3 grid((unsigned)tiles, (unsigned)((out_channels + 255) / 256));
  hipStream_t st = as_stream(stream);
  if (out_e4m3) {
    auto kern = k_conv3x3_fp8<true>;
    S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFp8));
    kern<<<grid, 256, kLdsFp8, st>>>((const uint8_t*)x_q, (const uint8_t*)weight_frag, scale, bias, out, (int)channels,
                                     (int)out_channels, relu, out_inv_scale, lt);
  } else {
    auto kern = k_conv3x3_fp8<false>;
    S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFp8));
    kern<<<grid, 256, kLdsFp8, st>>>((const uint8_t*)x_q, (const uint8_t*)weight_frag, scale, bias, out, (int)channels,
                                     (int)out_channels, relu, out_inv_scale, lt);
  }
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
