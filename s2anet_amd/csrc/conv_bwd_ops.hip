// Training side of the regular convolutions (FusedConv2d with own_grad): the per-step filter pack, the backward's
// preparation pass (ReLU mask + bias gradient) and the weight gradient.  The input gradient needs no kernel of its own: for a
// stride-1 3x3 / pad-1 or 1x1 convolution it is s2a_conv_nhwc_f16 on the transposed, 180-degree-rotated filter, which the pack
// below writes next to the forward filter.  The stride-2 layers (own_grad_strided) do need one -- k_conv_s2_bwd_input, from
// the same packed filter -- and take the weight gradient kernel at ST = 2.
#include <algorithm>

#include "common.hpp"

namespace s2a {
namespace {

using f16x8b = __attribute__((ext_vector_type(8))) _Float16;
using f32x16b = __attribute__((ext_vector_type(16))) float;
using s16x4b = __attribute__((ext_vector_type(4))) short;
using s16x8b = __attribute__((ext_vector_type(8))) short;

// ================================================================= filter pack (every step: the masters change)
// fragment order of k_pack_weight_frag (conv_ops.hip): [stage = cc*taps+t][och group of 64][mt 2][kk 4][lane 64][8 halfs],
// lane l, element j of fragment (mt,kk) = W[g*64 + mt*32 + (l&31)][cc*64 + kk*16 + 8*(l>>5) + j][t]
__device__ __forceinline__ void frag_coords(int64_t e, int O, int taps, int& och, int& k, int& t) {
  const int G = O / 64;
  const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), kk = (int)((e >> 9) & 3), mt = (int)((e >> 11) & 1);
  const int64_t r = e >> 12;
  const int g = (int)(r % G), st = (int)(r / G);
  t = st % taps;
  och = g * 64 + mt * 32 + (lane & 31);
  k = (st / taps) * 64 + kk * 16 + 8 * (lane >> 5) + j;
}

// fwd: the filter itself; dgrad: w'[c][o][t] = w[o][c][taps - 1 - t] (in/out channels swapped, taps rotated by 180 degrees)
template <typename T>
__global__ void k_conv_pack_train(const T* __restrict__ w, int O, int C, int taps, _Float16* __restrict__ fwd,
                                  _Float16* __restrict__ dgrad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)O * C * taps) return;
  int och, k, t;
  frag_coords(e, O, taps, och, k, t);
  fwd[e] = (_Float16)w[((int64_t)och * C + k) * taps + t];
  if (dgrad) {
    frag_coords(e, C, taps, och, k, t);                  // och: an input channel of w, k: an out channel of w
    dgrad[e] = (_Float16)w[((int64_t)k * C + och) * taps + (taps - 1 - t)];
  }
}

// ================================================================= backward preparation: ReLU mask + bias gradient
// one pass over grad_out [P][O]: g = out <= 0 ? 0 : grad_out (when out is given; selected, never multiplied: a NaN output
// passes the gradient, as torch's ReLU does) and, when the bias gradient is wanted, the
// per-channel f32 sums of g.  A workgroup owns a run of rows; thread (cx = tid & 7, ry = tid >> 3) takes the 8-channel
// vectors cx, cx + 8, ... of rows ry, ry + 32, ...; the 32 row-partials of a vector are summed in ry order, the workgroups'
// partials [workgroup][O] in workgroup order by k_conv_bwd_bias_final: no float atomics, the same bits every run.
constexpr int kPrepMaxBlocks = 256;
constexpr int kPrepRowsMin = 32;
inline int prep_blocks(int64_t P) {
  const int64_t nb = (P + kPrepRowsMin - 1) / kPrepRowsMin;
  return (int)(nb < kPrepMaxBlocks ? (nb < 1 ? 1 : nb) : kPrepMaxBlocks);
}

__global__ __launch_bounds__(256) void k_conv_bwd_prep(const _Float16* __restrict__ go, const _Float16* __restrict__ out,
                                                       _Float16* __restrict__ g, float* __restrict__ partial, int64_t P,
                                                       int O, int64_t rows_per_block) {
  __shared__ float s_red[32][8][8];
  const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < P ? r0 + rows_per_block : P;
  const int ovec = O / 8;
  for (int cv0 = 0; cv0 < ovec; cv0 += 8) {              // (ovec is a multiple of 8: every thread runs every trip)
    const int cv = cv0 + cx;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = 0.f;
    for (int64_t r = r0 + ry; r < r1; r += 32) {
      const int64_t at = r * O + cv * 8;
      f16x8b v = *reinterpret_cast<const f16x8b*>(go + at);
      if (out) {
        const f16x8b y = *reinterpret_cast<const f16x8b*>(out + at);
#pragma unroll
        for (int j = 0; j < 8; j++)
          if (y[j] <= (_Float16)0.f) v[j] = (_Float16)0.f;      // torch's rule: a NaN output passes the gradient
        if (g) *reinterpret_cast<f16x8b*>(g + at) = v;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) s[j] += (float)v[j];
    }
    if (partial) {
#pragma unroll
      for (int j = 0; j < 8; j++) s_red[ry][cx][j] = s[j];
      __syncthreads();
      if (tid < 64) {
        const int c8 = tid >> 3, j = tid & 7;
        float a = 0.f;
        for (int q = 0; q < 32; q++) a += s_red[q][c8][j];
        partial[(int64_t)blockIdx.x * O + (cv0 + c8) * 8 + j] = a;
      }
      __syncthreads();
    }
  }
}

template <typename T>
__global__ void k_conv_bwd_bias_final(const float* __restrict__ partial, int nblocks, int O, T* __restrict__ grad_bias) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= O) return;
  float a = 0.f;
  for (int b = 0; b < nblocks; b++) a += partial[(int64_t)b * O + o];
  grad_bias[o] = (T)a;
}

// ================================================================= weight gradient
// gw[o, c, ky, kx] = sum over (b, y, x) of g[b, y, x, o] * x[b, y + ky - 1, x + kx - 1, c]: k_dcn_bwd_weight (dcn_bwd_ops.hip)
// without the bilinear blend.  The contraction index is the POSITION, both operands sit in LDS as they sit in memory
// ([position][channel]) and are read "down the rows" with gfx950's transposing read.  The "columns" of a tap are the staged
// patch itself at an address shifted by the tap: no column tile is ever written.
//   * a workgroup owns one 64-channel chunk, one group of <= 256 out channels, one ROW of taps (ky; the 1x1 form has one tap)
//     and a slice of the position tiles (tile = slice, slice + ksplit, ...); its KS x [256 x 64] f32 results stay in
//     registers (8 waves x 32 out channels x KS taps x 2 accumulators) and go out once as a block of `partial`;
//   * 3x3: tile = 4 x 16 positions of one image, patch = rows ky - 1 .. ky + 2 of the tile, 18 pixels wide (zero outside the
//     image); 1x1: tile = 64 consecutive positions, patch = their rows;
//   * the NEXT tile's vectors are requested into registers before this tile's MFMAs;
//   * k_conv_bwd_weight_reduce sums the slices' blocks in slice order (a slice without a tile wrote exact zeros).
// EXEC: the transposing read needs all 64 lanes; a wave whose 32 out channels lie past the group takes no part AS A WHOLE
// (mwave), and nothing inside the matrix section depends on the lane.
// ST = 2 (the strided layers: 3x3 / s2 / p1 and 1x1 / s2): positions are those of the OUTPUT map [Ho, Wo], g is [B,Ho,Wo,O] and
// x stays [B,H,W,C]; tap (ky, kx) of position (oy, ox) samples x[2 oy + ky - 1][2 ox + kx - 1] (1x1: x[2 oy][2 ox]).
//   * a tap's 16 positions of a tile row are two pixels apart: read straight, rows 0/2 and 1/3 of a transposing read would
//     start on the same banks.  A patch row is therefore staged as TWO images, 33 pixels in all: pixels 0..15 the even columns
//     2 (tx0 + q), pixels 16..32 the odd columns 2 (tx0 + q) - 1, q = 0..16; kx = 1 reads the even image at q = p, kx = 0 the
//     odd one at q = p and kx = 2 the odd one at q = p + 1 -- consecutive pixels again, the stride-1 read pattern;
//   * the four patch rows are the input rows 2 (ty0 + r) + ky - 1;
//   * a block of `partial` is the gradient's own layout: partial[slice][o][c][ky][kx] (s2a_conv_backward_weight_s2_f16).
constexpr int kTPos = 64;                       // positions per tile
constexpr int kOGroup = 256;                    // out channels per workgroup
constexpr int kGoPitch = 576;                   // bytes per position of the g tile: 256 halfs + 64 (144 dwords = 16 mod 64: the four
                                                // rows of a transposing read start in four different 16-bank groups)
constexpr int kPatPitch = 192;                  // bytes per patch pixel: 64 halfs + 64 (48 dwords: rows start in banks 0, 48, 32, 16)
constexpr int kPatW = 18;                       // 16 + 2 halo columns
constexpr int kPatW2 = 33;                      // stride 2: 16 even + 17 odd columns
constexpr int kS2MaxSlices = 32;                // stride 2: a slice is a whole [O][C k k] f32 image, the reduce reads them all
constexpr int kWgradBlocks3 = 256, kWgradBlocks1 = 512;    // workgroups a launch aims at (3x3 / 1x1)

struct WgradGeom {
  int CC, OGN, nowner, ksplit, ostride;         // ostride: out-channel rows per partial block
  int64_t ntiles;
};
inline WgradGeom wgrad_geom(int64_t B, int64_t C, int64_t H, int64_t W, int64_t O, int ks) {
  WgradGeom q;
  q.CC = (int)(C / 64);
  q.OGN = (int)((O + kOGroup - 1) / kOGroup);
  q.nowner = q.CC * q.OGN * ks;
  const int target = ks == 3 ? kWgradBlocks3 : kWgradBlocks1;
  q.ksplit = target / q.nowner < 1 ? 1 : target / q.nowner;       // shapes only (never the tile count: a captured launch and
                                                                   // an eager one must sum in the same order)
  q.ostride = (int)(O < kOGroup ? O : kOGroup);
  q.ntiles = ks == 3 ? B * ((H + 3) / 4) * ((W + 15) / 16) : (B * H * W + kTPos - 1) / kTPos;
  return q;
}

template <int KS, int ST = 1>
__global__ __launch_bounds__(512, 2) void k_conv_bwd_weight(const _Float16* __restrict__ x,      // NHWC [B,H,W,C]
                                                           const _Float16* __restrict__ g,      // NHWC [B,Ho,Wo,O]
                                                           float* __restrict__ partial,         // [slice][owner][ostride][KS][64]
                                                           int B, int C, int H, int W, int O, int ksplit, int ostride,
                                                           int ntiles) {                        // (ST = 2: [slice][O][C][KS][KS])
  constexpr int kPatRow = ST == 2 ? kPatW2 : kPatW;
  constexpr int kPatPix = KS == 3 ? 4 * kPatRow : kTPos;
  constexpr int kPaVec = (kPatPix * 8 + 511) / 512;
  __shared__ __attribute__((aligned(16))) char s_go[kTPos * kGoPitch];
  __shared__ __attribute__((aligned(16))) char s_patch[kPatPix * kPatPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CC = C / 64, OGN = (O + kOGroup - 1) / kOGroup, nowner = CC * OGN * KS;
  const int owner = blockIdx.x % nowner, slice = blockIdx.x / nowner;
  const int ky = owner % KS, cc = (owner / KS) % CC, og = owner / (KS * CC);
  const int o0 = og * kOGroup, Og = min(kOGroup, O - o0);
  const bool mwave = wave * 32 < Og;            // (Og is a multiple of 64: the wave's 32 out channels exist, or none does)
  const int Ho = ST == 2 ? (H - 1) / 2 + 1 : H, Wo = ST == 2 ? (W - 1) / 2 + 1 : W;      // the map the positions live on
  const int64_t HW = (int64_t)Ho * Wo, P = (int64_t)B * HW, HWx = (int64_t)H * W;
  const int txn = (Wo + 15) / 16, tyn = (Ho + 3) / 4;

  f32x16b acc[KS][2];
#pragma unroll
  for (int a = 0; a < KS; a++)
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][c][r] = 0.f;

  // a thread's vectors (16 bytes each): g tile = 64 positions x 32 vectors (those of the group's channels), patch = kPatPix x 8
  f16x8b gv[4], pvv[kPaVec];
  auto issue = [&](int tile) {
    int b = 0, ty0 = 0, tx0 = 0;
    if (KS == 3) {
      const int r = tile % (tyn * txn);
      b = tile / (tyn * txn); ty0 = (r / txn) * 4; tx0 = (r % txn) * 16;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int v = tid + 512 * i, pos = v >> 5, ch = (v & 31) * 8;
      gv[i] = f16x8b{};
      if (ch < Og) {
        if (KS == 3) {
          const int y = ty0 + (pos >> 4), xq = tx0 + (pos & 15);
          if (y < Ho && xq < Wo) gv[i] = *reinterpret_cast<const f16x8b*>(g + ((int64_t)b * HW + (int64_t)y * Wo + xq) * O + o0 + ch);
        } else {
          const int64_t n = (int64_t)tile * kTPos + pos;
          if (n < P) gv[i] = *reinterpret_cast<const f16x8b*>(g + n * O + o0 + ch);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kPaVec; i++) {
      const int v = tid + 512 * i, pix = v >> 3, q = (v & 7) * 8;
      pvv[i] = f16x8b{};
      if (v < kPatPix * 8) {
        if (KS == 3) {
          const int pr = pix / kPatRow, pc = pix % kPatRow;
          const int yy = ST == 2 ? 2 * (ty0 + pr) + ky - 1 : ty0 + pr + ky - 1;
          const int xx = ST == 2 ? (pc < 16 ? 2 * (tx0 + pc) : 2 * (tx0 + pc - 16) - 1) : tx0 + pc - 1;
          if (yy >= 0 && yy < H && xx >= 0 && xx < W)
            pvv[i] = *reinterpret_cast<const f16x8b*>(x + ((int64_t)b * HWx + (int64_t)yy * W + xx) * C + cc * 64 + q);
        } else {
          const int64_t n = (int64_t)tile * kTPos + pix;
          if (n < P) {
            int64_t at = n;
            if (ST == 2) {
              const int64_t bi = n / HW;
              const int rr = (int)(n - bi * HW);
              at = bi * HWx + (int64_t)(2 * (rr / Wo)) * W + 2 * (rr % Wo);
            }
            pvv[i] = *reinterpret_cast<const f16x8b*>(x + at * C + cc * 64 + q);
          }
        }
      }
    }
  };
  auto land = [&]() {                            // (zeros included: every byte the matrix section reads is rewritten per tile)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int v = tid + 512 * i;
      if ((v & 31) * 8 < Og) *reinterpret_cast<f16x8b*>(s_go + (v >> 5) * kGoPitch + (v & 31) * 16) = gv[i];
    }
#pragma unroll
    for (int i = 0; i < kPaVec; i++) {
      const int v = tid + 512 * i;
      if (v < kPatPix * 8) *reinterpret_cast<f16x8b*>(s_patch + (v >> 3) * kPatPitch + (v & 7) * 16) = pvv[i];
    }
  };

  int tile = slice;
  if (tile < ntiles) issue(tile);
  for (; tile < ntiles; tile += ksplit) {
    __syncthreads();                             // the previous tile's operands have been read
    land();
    __syncthreads();
    if (tile + ksplit < ntiles) issue(tile + ksplit);      // in flight under the MFMAs
    // gw tiles += g^T . patch over the 64 positions: lane 16 gq + 4 qq + pp supplies row qq, elements 4 pp .. 4 pp + 3 of its
    // group's 4 x 16 block and receives column (lane & 15) of the four rows; group gq covers rows 8 (gq >> 1) + 4 r .. + 3 of
    // the 16-position step ks and columns 16 (gq & 1) .. + 15.  Position 16 ks + p of a 3x3 tile is tile row ks, column p:
    // its tap-kx sample is patch pixel ks * 18 + p + kx (the patch rows are already shifted by ky).
    // 3x3: tile positions outside the image hold g = 0, but their tap-shifted patch pixels can lie INSIDE it, and 0 * inf
    // is NaN.  Such positions leave the contraction: a tile row below the image is skipped (ks >= rows_in), and in a tile
    // that crosses the right edge the B elements of the columns past it are cleared (a lane's 8 elements of a fragment are
    // columns 8 (gq >> 1) .. + 7 of tile row ks).  Both conditions are uniform; finite data sums the same bits as before.
    int rows_in = 4, cols_in = 16;
    if (KS == 3) {
      const int r = tile % (tyn * txn);
      rows_in = min(4, Ho - (r / txn) * 4);
      cols_in = min(16, Wo - (r % txn) * 16);
    }
    if (mwave) {
      const int gq = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
      const int prow = 8 * (gq >> 1) + qq;
      s16x8b keep;
#pragma unroll
      for (int j = 0; j < 8; j++) keep[j] = 8 * (gq >> 1) + j < cols_in ? (short)-1 : (short)0;
      const char* a_base = s_go + prow * kGoPitch + (wave * 32 + 16 * (gq & 1) + 4 * pp) * 2;
      const char* b_base = s_patch + prow * kPatPitch + (16 * (gq & 1) + 4 * pp) * 2;
      auto tr = [&](const char* p) {
        return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4b*)p);
      };
      auto frag = [&](const char* p, int pitch) {
        const s16x4b lo = tr(p), hi = tr(p + 4 * pitch);
        const s16x8b v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(f16x8b, v);
      };
#pragma unroll
      for (int ks = 0; ks < kTPos / 16; ks++) {
        if (KS == 3 && ks >= rows_in) continue;
        const f16x8b A = frag(a_base + ks * 16 * kGoPitch, kGoPitch);
#pragma unroll
        for (int tl = 0; tl < KS; tl++)
#pragma unroll
          for (int ct = 0; ct < 2; ct++) {
            const int pix0 = KS != 3 ? ks * 16 : ST == 2 ? ks * kPatW2 + (tl == 1 ? 0 : 16 + (tl >> 1)) : ks * kPatW + tl;
            f16x8b Bf = frag(b_base + pix0 * kPatPitch + ct * 64, kPatPitch);
            if (KS == 3 && cols_in < 16) Bf = __builtin_bit_cast(f16x8b, __builtin_bit_cast(s16x8b, Bf) & keep);
            acc[tl][ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, Bf, acc[tl][ct], 0, 0, 0);
          }
      }
    }
  }
  // results: rows = out channels (4 consecutive per register quad), columns = channels of the chunk
  if (mwave) {
    float* part = ST == 2 ? partial + (int64_t)slice * O * C * (KS * KS)
                          : partial + (int64_t)blockIdx.x * ostride * (KS * 64);      // (blockIdx = slice * nowner + owner)
#pragma unroll
    for (int tl = 0; tl < KS; tl++)
#pragma unroll
      for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int o = wave * 32 + 8 * (r >> 2) + (r & 3) + 4 * (lane >> 5);
          if (ST == 2)
            part[((int64_t)(o0 + o) * C + cc * 64 + ct * 32 + (lane & 31)) * (KS * KS) + ky * KS + tl] = acc[tl][ct][r];
          else
            part[(o * KS + tl) * 64 + ct * 32 + (lane & 31)] = acc[tl][ct][r];
        }
  }
}

// gw[o][c][ky][kx] = the slices' blocks summed in slice order; thread index = (o, cc, ky, kx, c of the chunk)
template <int KS, typename T>
__global__ void k_conv_bwd_weight_reduce(const float* __restrict__ partial, int C, int O, int ksplit, int ostride,
                                         T* __restrict__ gw) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)O * C * KS * KS) return;
  const int CC = C / 64, OGN = (O + kOGroup - 1) / kOGroup, nowner = CC * OGN * KS;
  const int c = (int)(e & 63);
  int64_t r = e >> 6;
  const int kx = (int)(r % KS); r /= KS;
  const int ky = (int)(r % KS); r /= KS;
  const int cc = (int)(r % CC);
  const int o = (int)(r / CC);
  const int owner = ((o / kOGroup) * CC + cc) * KS + ky;
  const float* p = partial + ((int64_t)owner * ostride + (o % kOGroup)) * (KS * 64) + kx * 64 + c;
  const int64_t step = (int64_t)nowner * ostride * (KS * 64);
  float a = 0.f;
  for (int s = 0; s < ksplit; s++) a += p[s * step];
  gw[(((int64_t)o * C + cc * 64 + c) * KS + ky) * KS + kx] = (T)a;
}

// stride 2: out[e] = partial[0][e] + partial[1][e] + ... in slice order, f32 or (one rounding) f16
template <typename T>
__global__ void k_conv_bwd_weight_s2_reduce(const float* __restrict__ partial, int slices, int64_t count, T* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  float a = 0.f;
  for (int s = 0; s < slices; s++) a += partial[s * count + e];
  out[e] = (T)a;
}

// ================================================================= input gradient, stride 2
// A stride-2 convolution's input gradient is no stride-1 convolution of g.  Input pixel (y, x) = (2 i + py, 2 j + px) of the
// 3x3 / p1 form receives, by parity class (g outside [0,Ho) x [0,Wo) takes no part),
//   (0,0)  w[1,1] g[i,j]
//   (0,1)  w[1,0] g[i,j+1] + w[1,2] g[i,j]
//   (1,0)  w[0,1] g[i+1,j] + w[2,1] g[i,j]
//   (1,1)  w[0,0] g[i+1,j+1] + w[0,2] g[i+1,j] + w[2,0] g[i,j+1] + w[2,2] g[i,j]
// each w[ky,kx] g being the [C x O] . [O] product over the out channels: nine tap products per 2 x 2 input pixels, the
// forward's count.  The 1x1 form is class (0,0) alone with its one tap; its other three pixels are written as +0.
//   * a workgroup owns 4 x 16 quads (2 x 2 input pixels each) of one image and 64 input channels; wave (mt, half) holds
//     channels 32 mt .. + 31 of the quads 32 half .. + 31, one 32 x 32 f32 accumulator per class;
//   * per 64-out-channel chunk the g patch (5 x 17 pixels, 4 x 16 for 1x1; zeros outside the map, never loaded) is staged in LDS
//     at a 144-byte pitch (36 dwords: the 16 pixels of a half-wave's 16-byte reads cover the 64 banks once); a lane's B
//     fragment is 16 bytes of its quad's neighbour pixel;
//   * the filter fragments come straight from s2a_conv_pack_weight_train's input-gradient filter (w'[c][o][8 - t], fragment
//     order of frag_coords with the INPUT channels as rows): tap (ky, kx) of w is stage oc * taps + (taps - 1 - (3 ky + kx));
//   * a quad whose neighbour row or column is outside the map keeps its accumulator instead of adding w . 0 (selected per
//     lane behind the MFMA, in tiles on the bottom / right edge only; the branch is uniform).  Fixed order, no atomics.
constexpr int kDgPitch = 144;

template <int KS>
__global__ __launch_bounds__(256) void k_conv_s2_bwd_input(const _Float16* __restrict__ g,        // NHWC [B,Ho,Wo,O]
                                                           const _Float16* __restrict__ wpk,      // input-gradient filter
                                                           _Float16* __restrict__ gx,             // NHWC [B,H,W,C]
                                                           int C, int H, int W, int O) {
  constexpr int HALO = KS == 3 ? 1 : 0, PC = 16 + HALO, NPIX = (4 + HALO) * PC, NVEC = (NPIX * 8 + 255) / 256;
  constexpr int NCLS = KS == 3 ? 4 : 1, TAPS = KS * KS;
  __shared__ __attribute__((aligned(16))) char s_g[NPIX * kDgPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt = wave & 1, half = wave >> 1;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, txn = (Wo + 15) / 16, tyn = (Ho + 3) / 4;
  const int rt = blockIdx.x % (tyn * txn), b = blockIdx.x / (tyn * txn);
  const int i0 = (rt / txn) * 4, j0 = (rt % txn) * 16, cg = blockIdx.y, G = C / 64;
  const int n = half * 32 + (lane & 31), ti = n >> 4, tj = n & 15;      // the lane's quad of the tile
  const int qi = i0 + ti, qj = j0 + tj;
  const bool vi = qi + 1 < Ho, vj = qj + 1 < Wo;                        // the quad's lower / right neighbour exists
  const bool edge = i0 + 4 >= Ho || j0 + 16 >= Wo;                      // (uniform) some quad of the tile lacks one

  f32x16b acc[NCLS];
#pragma unroll
  for (int a = 0; a < NCLS; a++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[a][r] = 0.f;

  auto mac = [&](f32x16b& d, const f16x8b& A, const f16x8b& Bf, bool ok) {
    const f32x16b t = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, Bf, d, 0, 0, 0);
    if (KS == 3 && edge) {
#pragma unroll
      for (int r = 0; r < 16; r++) d[r] = ok ? t[r] : d[r];
    } else {
      d = t;
    }
  };

  // a thread's vectors of the g patch are requested one chunk ahead, the filter fragments of a k-step (16 out channels, TAPS x
  // 16 bytes a lane) one step ahead: both are in flight under the MFMAs
  f16x8b gv[NVEC];
  auto issue = [&](int oc) {
#pragma unroll
    for (int i = 0; i < NVEC; i++) {
      const int v = tid + 256 * i, pix = v >> 3, q = (v & 7) * 8, y = i0 + pix / PC, xq = j0 + pix % PC;
      gv[i] = f16x8b{};
      if (v < NPIX * 8 && y < Ho && xq < Wo)
        gv[i] = *reinterpret_cast<const f16x8b*>(g + (((int64_t)b * Ho + y) * Wo + xq) * O + oc * 64 + q);
    }
  };
  auto land = [&]() {                            // (zeros included: every byte the matrix section reads is rewritten per chunk)
#pragma unroll
    for (int i = 0; i < NVEC; i++) {
      const int v = tid + 256 * i;
      if (v < NPIX * 8) *reinterpret_cast<f16x8b*>(s_g + (v >> 3) * kDgPitch + (v & 7) * 16) = gv[i];
    }
  };
  // fragment (stage = oc TAPS + t, cg, mt, kk) of the pack: 64 lanes x 8 halfs; tap (ky, kx) of w is t = TAPS - 1 - (ky KS + kx)
  const _Float16* wbase = wpk + ((int64_t)cg * 2 + mt) * 4 * 512 + lane * 8;
  const int steps = O / 16;
  f16x8b wa[TAPS], wn[TAPS];
  auto wload = [&](f16x8b(&dst)[TAPS], int step) {
#pragma unroll
    for (int t = 0; t < TAPS; t++)
      dst[t] = *reinterpret_cast<const f16x8b*>(wbase + ((int64_t)((step >> 2) * TAPS + t) * G * 8 + (step & 3)) * 512);
  };
  auto tap = [&](int ky, int kx) -> const f16x8b& { return wa[TAPS - 1 - (ky * KS + kx)]; };

  issue(0);
  wload(wa, 0);
  for (int oc = 0; oc < O / 64; oc++) {
    __syncthreads();                             // the previous chunk's patch has been read
    land();
    __syncthreads();
    if (oc + 1 < O / 64) issue(oc + 1);
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      wload(wn, min(oc * 4 + kk + 1, steps - 1));           // (the last step asks for itself again: in bounds, not used)
      const char* bp = s_g + (ti * PC + tj) * kDgPitch + kk * 32 + (lane >> 5) * 16;
      const f16x8b g00 = *reinterpret_cast<const f16x8b*>(bp);
      if (KS == 1) {
        mac(acc[0], tap(0, 0), g00, true);
      } else {
        const f16x8b g01 = *reinterpret_cast<const f16x8b*>(bp + kDgPitch);
        const f16x8b g10 = *reinterpret_cast<const f16x8b*>(bp + PC * kDgPitch);
        const f16x8b g11 = *reinterpret_cast<const f16x8b*>(bp + (PC + 1) * kDgPitch);
        mac(acc[0], tap(1, 1), g00, true);
        mac(acc[1], tap(1, 0), g01, vj);
        mac(acc[1], tap(1, 2), g00, true);
        mac(acc[2], tap(0, 1), g10, vi);
        mac(acc[2], tap(2, 1), g00, true);
        mac(acc[3], tap(0, 0), g11, vi && vj);
        mac(acc[3], tap(0, 2), g10, vi);
        mac(acc[3], tap(2, 0), g01, vj);
        mac(acc[3], tap(2, 2), g00, true);
      }
#pragma unroll
      for (int t = 0; t < TAPS; t++) wa[t] = wn[t];
    }
  }
  // results: column (lane & 31) = the lane's quad, register quad rq = channels 8 rq + 4 (lane >> 5) .. + 3 of the wave's 32
  if (qi < Ho && qj < Wo) {
#pragma unroll
    for (int cls = 0; cls < 4; cls++) {
      const int y = 2 * qi + (cls >> 1), xq = 2 * qj + (cls & 1);
      if (y < H && xq < W) {
        _Float16* dst = gx + (((int64_t)b * H + y) * W + xq) * C + cg * 64 + mt * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int rq = 0; rq < 4; rq++) {
          using f16x4b = __attribute__((ext_vector_type(4))) _Float16;
          f16x4b o = f16x4b{};                   // (1x1: the three other pixels of the quad are +0)
          if (cls < NCLS) {
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = (_Float16)acc[cls < NCLS ? cls : 0][4 * rq + j];
          }
          *reinterpret_cast<f16x4b*>(dst + 8 * rq) = o;
        }
      }
    }
  }
}

inline bool dtype_ok(int d) { return d == S2A_DTYPE_F32 || d == S2A_DTYPE_F16; }
inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" int s2a_conv_pack_weight_train(const void* weight, int weight_dtype, int64_t out_channels, int64_t channels,
                                          int ksize, void* packed_fwd, void* packed_dgrad, s2a_stream_t stream) {
  S2A_CHECK_ARG(ksize == 3 || ksize == 1, "conv_pack_weight_train: kernel size must be 1 or 3");
  S2A_CHECK_ARG(dtype_ok(weight_dtype), "conv_pack_weight_train: weight dtype must be f32 or f16");
  S2A_CHECK_ARG(out_channels > 0 && channels > 0 && out_channels % 64 == 0 && channels % 64 == 0,
                "conv_pack_weight_train: bad shape (channel counts must be positive multiples of 64)");
  S2A_CHECK_ARG((uint64_t)out_channels * channels * ksize * ksize * 4 < (1ull << 31),
                "conv_pack_weight_train: filter too large for 32-bit offsets");
  S2A_CHECK_ARG(weight && packed_fwd, "conv_pack_weight_train: NULL tensor");
  S2A_CHECK_ARG(aligned16(weight) && aligned16(packed_fwd) && aligned16(packed_dgrad),
                "conv_pack_weight_train: tensors must be 16-byte aligned");
  const int taps = ksize * ksize;
  const int64_t wtot = out_channels * channels * taps;
  const unsigned blocks = (unsigned)((wtot + 255) / 256);
  hipStream_t st = as_stream(stream);
  if (weight_dtype == S2A_DTYPE_F32)
    k_conv_pack_train<float><<<blocks, 256, 0, st>>>((const float*)weight, (int)out_channels, (int)channels, taps,
                                                     (_Float16*)packed_fwd, (_Float16*)packed_dgrad);
  else
    k_conv_pack_train<_Float16><<<blocks, 256, 0, st>>>((const _Float16*)weight, (int)out_channels, (int)channels, taps,
                                                        (_Float16*)packed_fwd, (_Float16*)packed_dgrad);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" size_t s2a_conv_backward_prep_f16_workspace_bytes(int64_t positions, int64_t out_channels) {
  if (positions <= 0 || out_channels <= 0 || out_channels % 64 != 0 || (uint64_t)positions * out_channels * 2 >= (1ull << 31))
    return 0;
  return align_up((size_t)prep_blocks(positions) * out_channels * sizeof(float));
}

extern "C" int s2a_conv_backward_prep_f16(const void* grad_out, const void* out, void* g, void* grad_bias,
                                          int grad_bias_dtype, int64_t positions, int64_t out_channels, void* workspace,
                                          size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(positions >= 0 && out_channels > 0 && out_channels % 64 == 0,
                "conv_backward_prep: bad shape (out_channels must be a positive multiple of 64)");
  S2A_CHECK_ARG((uint64_t)positions * out_channels * 2 < (1ull << 31), "conv_backward_prep: tensor too large for 32-bit offsets");
  S2A_CHECK_ARG(!grad_bias || dtype_ok(grad_bias_dtype), "conv_backward_prep: bias gradient dtype must be f32 or f16");
  S2A_CHECK_ARG(!g || out, "conv_backward_prep: a masked gradient needs the forward output");
  if (positions == 0 || (!grad_bias && !g)) return S2A_OK;            // nothing to write
  S2A_CHECK_ARG(grad_out, "conv_backward_prep: NULL tensor");
  S2A_CHECK_ARG(aligned16(grad_out) && aligned16(out) && aligned16(g) && ((uintptr_t)grad_bias % 4) == 0 && aligned16(workspace),
                "conv_backward_prep: tensors must be 16-byte aligned");
  const int nb = prep_blocks(positions);
  float* partial = nullptr;
  if (grad_bias) {
    S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_conv_backward_prep_f16_workspace_bytes(positions, out_channels),
                        "conv_backward_prep_f16");
    partial = (float*)workspace;
  }
  hipStream_t st = as_stream(stream);
  const int64_t rows = (positions + nb - 1) / nb;
  k_conv_bwd_prep<<<nb, 256, 0, st>>>((const _Float16*)grad_out, (const _Float16*)out, (_Float16*)g, partial, positions,
                                      (int)out_channels, rows);
  S2A_LAUNCH_CHECK();
  if (grad_bias) {
    const unsigned fb = (unsigned)((out_channels + 255) / 256);
    if (grad_bias_dtype == S2A_DTYPE_F32)
      k_conv_bwd_bias_final<float><<<fb, 256, 0, st>>>(partial, nb, (int)out_channels, (float*)grad_bias);
    else
      k_conv_bwd_bias_final<_Float16><<<fb, 256, 0, st>>>(partial, nb, (int)out_channels, (_Float16*)grad_bias);
    S2A_LAUNCH_CHECK();
  }
  return S2A_OK;
}

static bool wgrad_shape_ok(int64_t B, int64_t C, int64_t H, int64_t W, int64_t O, int ksize) {
  return B >= 0 && C > 0 && H > 0 && W > 0 && O > 0 && (ksize == 3 || ksize == 1) && C % 64 == 0 && O % 64 == 0 &&
         H < 32000 && W < 32000 && B < (1ll << 31) && C < (1ll << 24) && O < (1ll << 24) &&
         (uint64_t)B * H * W * C * 2 < (1ull << 31) && (uint64_t)B * H * W * O * 2 < (1ull << 31) &&
         (uint64_t)O * C * ksize * ksize * 4 < (1ull << 31);
}

extern "C" size_t s2a_conv_backward_weight_f16_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                               int64_t out_channels, int ksize) {
  if (!wgrad_shape_ok(batch, channels, height, width, out_channels, ksize) || batch == 0) return 0;
  const WgradGeom q = wgrad_geom(batch, channels, height, width, out_channels, ksize);
  // (the launch writes ksplit * nowner blocks, at most the count it aims at while nowner is below it; the query declares that
  // count itself, so that it never shrinks when a size grows: 255 blocks at 64 channels, 252 at 128)
  const size_t aim = ksize == 3 ? kWgradBlocks3 : kWgradBlocks1;
  const size_t blocks = std::max((size_t)q.ksplit * q.nowner, std::max(aim, (size_t)q.nowner));
  return align_up(blocks * q.ostride * ksize * 64 * sizeof(float));
}

extern "C" int s2a_conv_backward_weight_f16(const void* x, const void* g, void* grad_weight, int grad_dtype, int64_t batch,
                                            int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                                            void* workspace, size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(ksize == 3 || ksize == 1, "conv_backward_weight: kernel size must be 1 or 3");
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0 && height > 0 && width > 0, "conv_backward_weight: bad shape");
  S2A_CHECK_ARG(channels % 64 == 0 && out_channels % 64 == 0, "conv_backward_weight: channel counts must be multiples of 64");
  S2A_CHECK_ARG(wgrad_shape_ok(batch, channels, height, width, out_channels, ksize),
                "conv_backward_weight: tensor too large for 32-bit offsets");
  S2A_CHECK_ARG(dtype_ok(grad_dtype), "conv_backward_weight: gradient dtype must be f32 or f16");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && g && grad_weight, "conv_backward_weight: NULL tensor");
  S2A_CHECK_ARG(aligned16(x) && aligned16(g) && aligned16(grad_weight) && aligned16(workspace),
                "conv_backward_weight: tensors must be 16-byte aligned");
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes,
                      s2a_conv_backward_weight_f16_workspace_bytes(batch, channels, height, width, out_channels, ksize),
                      "conv_backward_weight_f16");
  const WgradGeom q = wgrad_geom(batch, channels, height, width, out_channels, ksize);
  S2A_CHECK_ARG(q.ntiles < (1ll << 31) && (int64_t)q.ksplit * q.nowner < (1ll << 31), "conv_backward_weight: too many tiles");
  hipStream_t st = as_stream(stream);
  const _Float16 *X = (const _Float16*)x, *G = (const _Float16*)g;
  float* partial = (float*)workspace;
  const unsigned grid = (unsigned)(q.ksplit * q.nowner);
  const int B = (int)batch, C = (int)channels, H = (int)height, W = (int)width, O = (int)out_channels;
  const int64_t total = out_channels * channels * ksize * ksize;
  const unsigned rb = (unsigned)((total + 255) / 256);
  if (ksize == 3) {
    k_conv_bwd_weight<3><<<grid, 512, 0, st>>>(X, G, partial, B, C, H, W, O, q.ksplit, q.ostride, (int)q.ntiles);
    S2A_LAUNCH_CHECK();
    if (grad_dtype == S2A_DTYPE_F32)
      k_conv_bwd_weight_reduce<3, float><<<rb, 256, 0, st>>>(partial, C, O, q.ksplit, q.ostride, (float*)grad_weight);
    else
      k_conv_bwd_weight_reduce<3, _Float16><<<rb, 256, 0, st>>>(partial, C, O, q.ksplit, q.ostride, (_Float16*)grad_weight);
  } else {
    k_conv_bwd_weight<1><<<grid, 512, 0, st>>>(X, G, partial, B, C, H, W, O, q.ksplit, q.ostride, (int)q.ntiles);
    S2A_LAUNCH_CHECK();
    if (grad_dtype == S2A_DTYPE_F32)
      k_conv_bwd_weight_reduce<1, float><<<rb, 256, 0, st>>>(partial, C, O, q.ksplit, q.ostride, (float*)grad_weight);
    else
      k_conv_bwd_weight_reduce<1, _Float16><<<rb, 256, 0, st>>>(partial, C, O, q.ksplit, q.ostride, (_Float16*)grad_weight);
  }
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

// ================================================================= stride 2 (3x3 / p1 and 1x1): input and weight gradient
namespace {
// what is wrong with a strided problem, or nullptr: the checks the entry points and the slices query share
const char* s2_shape_problem(int64_t B, int64_t C, int64_t H, int64_t W, int64_t O, int ksize) {
  if (ksize != 3 && ksize != 1) return "kernel size must be 1 or 3";
  if (!(B >= 0 && C > 0 && O > 0 && H > 0 && W > 0)) return "bad shape";
  if (C % 64 != 0 || O % 64 != 0) return "channel counts must be multiples of 64";
  if (ksize == 3 && O % 128 != 0) return "3x3 stride 2 needs out_channels % 128 == 0";
  const uint64_t Ho = (uint64_t)(H - 1) / 2 + 1, Wo = (uint64_t)(W - 1) / 2 + 1;
  if (!(H < 32000 && W < 32000 && B < (1ll << 31) && C < (1ll << 24) && O < (1ll << 24) &&
        (uint64_t)B * H * W * C * 2 < (1ull << 31) && (uint64_t)B * Ho * Wo * O * 2 < (1ull << 31) &&
        (uint64_t)O * C * ksize * ksize * 4 < (1ull << 31)))
    return "tensor too large for 32-bit offsets (2^31 bytes or more)";
  return nullptr;
}
}  // namespace

extern "C" int s2a_conv_backward_input_s2_f16(const void* g, const void* packed_dgrad, void* grad_input, int64_t batch,
                                              int64_t channels, int64_t height, int64_t width, int64_t out_channels,
                                              int ksize, s2a_stream_t stream) {
  const char* problem = s2_shape_problem(batch, channels, height, width, out_channels, ksize);
  S2A_CHECK_ARG(!problem, "conv_backward_input_s2: %s", problem);
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(g && packed_dgrad && grad_input, "conv_backward_input_s2: NULL tensor");
  S2A_CHECK_ARG(aligned16(g) && aligned16(packed_dgrad) && aligned16(grad_input),
                "conv_backward_input_s2: tensors must be 16-byte aligned");
  const int64_t Ho = (height - 1) / 2 + 1, Wo = (width - 1) / 2 + 1;
  const int64_t tiles = batch * ((Ho + 3) / 4) * ((Wo + 15) / 16);
  S2A_CHECK_ARG(tiles < (1ll << 31) && channels / 64 < 65536, "conv_backward_input_s2: too many tiles");
  const dim3 grid((unsigned)tiles, (unsigned)(channels / 64));
  hipStream_t st = as_stream(stream);
  const int C = (int)channels, H = (int)height, W = (int)width, O = (int)out_channels;
  if (ksize == 3)
    k_conv_s2_bwd_input<3><<<grid, 256, 0, st>>>((const _Float16*)g, (const _Float16*)packed_dgrad, (_Float16*)grad_input, C, H, W, O);
  else
    k_conv_s2_bwd_input<1><<<grid, 256, 0, st>>>((const _Float16*)g, (const _Float16*)packed_dgrad, (_Float16*)grad_input, C, H, W, O);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_conv_backward_weight_s2_slices(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                  int64_t out_channels, int ksize) {
  if (s2_shape_problem(batch, channels, height, width, out_channels, ksize) || batch == 0) return 0;
  const WgradGeom q = wgrad_geom(batch, channels, (height - 1) / 2 + 1, (width - 1) / 2 + 1, out_channels, ksize);
  return std::min(q.ksplit, kS2MaxSlices);      // (shapes only, as ksplit)
}

extern "C" int s2a_conv_backward_weight_s2_f16(const void* x, const void* g, void* partial, int slices, int64_t batch,
                                               int64_t channels, int64_t height, int64_t width, int64_t out_channels,
                                               int ksize, s2a_stream_t stream) {
  const char* problem = s2_shape_problem(batch, channels, height, width, out_channels, ksize);
  S2A_CHECK_ARG(!problem, "conv_backward_weight_s2: %s", problem);
  S2A_CHECK_ARG(batch > 0, "conv_backward_weight_s2: bad shape (an empty batch has no slices)");
  const int want = s2a_conv_backward_weight_s2_slices(batch, channels, height, width, out_channels, ksize);
  S2A_CHECK_ARG(slices == want, "conv_backward_weight_s2: slices is %d, s2a_conv_backward_weight_s2_slices answers %d", slices, want);
  S2A_CHECK_ARG(x && g && partial, "conv_backward_weight_s2: NULL tensor");
  S2A_CHECK_ARG(aligned16(x) && aligned16(g) && aligned16(partial), "conv_backward_weight_s2: tensors must be 16-byte aligned");
  const WgradGeom q = wgrad_geom(batch, channels, (height - 1) / 2 + 1, (width - 1) / 2 + 1, out_channels, ksize);
  S2A_CHECK_ARG(q.ntiles < (1ll << 31), "conv_backward_weight_s2: too many tiles");
  hipStream_t st = as_stream(stream);
  const unsigned grid = (unsigned)(slices * q.nowner);
  const int B = (int)batch, C = (int)channels, H = (int)height, W = (int)width, O = (int)out_channels;
  if (ksize == 3)
    k_conv_bwd_weight<3, 2><<<grid, 512, 0, st>>>((const _Float16*)x, (const _Float16*)g, (float*)partial, B, C, H, W, O, slices,
                                                  q.ostride, (int)q.ntiles);
  else
    k_conv_bwd_weight<1, 2><<<grid, 512, 0, st>>>((const _Float16*)x, (const _Float16*)g, (float*)partial, B, C, H, W, O, slices,
                                                  q.ostride, (int)q.ntiles);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_conv_backward_weight_s2_reduce(const void* partial, int slices, int64_t count, void* out, int out_dtype,
                                                  s2a_stream_t stream) {
  S2A_CHECK_ARG(slices > 0 && count >= 0, "conv_backward_weight_s2_reduce: bad shape");
  S2A_CHECK_ARG((uint64_t)count * 4 < (1ull << 31), "conv_backward_weight_s2_reduce: tensor too large for 32-bit offsets");
  S2A_CHECK_ARG(dtype_ok(out_dtype), "conv_backward_weight_s2_reduce: output dtype must be f32 or f16");
  if (count == 0) return S2A_OK;
  S2A_CHECK_ARG(partial && out, "conv_backward_weight_s2_reduce: NULL tensor");
  S2A_CHECK_ARG(aligned16(partial) && aligned16(out), "conv_backward_weight_s2_reduce: tensors must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const unsigned rb = (unsigned)((count + 255) / 256);
  if (out_dtype == S2A_DTYPE_F32)
    k_conv_bwd_weight_s2_reduce<float><<<rb, 256, 0, st>>>((const float*)partial, slices, count, (float*)out);
  else
    k_conv_bwd_weight_s2_reduce<_Float16><<<rb, 256, 0, st>>>((const float*)partial, slices, count, (_Float16*)out);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

// ================================================================= FPN top-down: the gradient of the nearest 2x up-sampling
namespace {
// one thread = 8 maps of one coarse pixel: ((g[2i,2j] + g[2i,2j+1]) + g[2i+1,2j]) + g[2i+1,2j+1] over f32, one rounding
__global__ void k_sum_pool2x2(const _Float16* __restrict__ g, _Float16* __restrict__ out, int Hh, int Wh, int O8, int64_t items) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= items) return;
  const int c = (int)(e % O8);
  const int64_t pix = e / O8;
  const int j = (int)(pix % Wh), i = (int)((pix / Wh) % Hh);
  const int64_t b = pix / ((int64_t)Wh * Hh);
  const int64_t row = (int64_t)2 * Wh * O8 * 8;                               // halfs per row of g
  const _Float16* src = g + ((b * 2 * Hh + 2 * i) * 2 * Wh + 2 * j) * (int64_t)O8 * 8 + c * 8;
  const f16x8b a0 = *reinterpret_cast<const f16x8b*>(src), a1 = *reinterpret_cast<const f16x8b*>(src + O8 * 8);
  const f16x8b b0 = *reinterpret_cast<const f16x8b*>(src + row), b1 = *reinterpret_cast<const f16x8b*>(src + row + O8 * 8);
  f16x8b r;
#pragma unroll
  for (int k = 0; k < 8; k++) r[k] = (_Float16)((((float)a0[k] + (float)a1[k]) + (float)b0[k]) + (float)b1[k]);
  *reinterpret_cast<f16x8b*>(out + e * 8) = r;
}
}  // namespace

extern "C" int s2a_sum_pool2x2_f16(const void* g, void* out, int64_t batch, int64_t height, int64_t width, int64_t channels,
                                   s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && height > 0 && width > 0 && channels > 0, "sum_pool2x2: bad shape");
  S2A_CHECK_ARG(height % 2 == 0 && width % 2 == 0, "sum_pool2x2: the map must be exactly twice the coarse map");
  S2A_CHECK_ARG(channels % 8 == 0, "sum_pool2x2: the channel count must be a multiple of 8");
  S2A_CHECK_ARG(height < (1ll << 24) && width < (1ll << 24) && channels < (1ll << 24) && batch < (1ll << 31) &&
                (uint64_t)batch * height * width * channels * 2 < (1ull << 31), "sum_pool2x2: tensor too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(g && out, "sum_pool2x2: NULL tensor");
  S2A_CHECK_ARG(aligned16(g) && aligned16(out), "sum_pool2x2: tensors must be 16-byte aligned");
  const int64_t items = batch * (height / 2) * (width / 2) * (channels / 8);
  k_sum_pool2x2<<<(unsigned)((items + 255) / 256), 256, 0, as_stream(stream)>>>((const _Float16*)g, (_Float16*)out, (int)(height / 2),
                                                                                (int)(width / 2), (int)(channels / 8), items);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
