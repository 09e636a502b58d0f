// Dense f16 convolutions for MI355X (gfx950): the 3x3 / 1x1 layers of the trunk, the FPN and the head towers.
//
// k_conv_f16 (3x3 and 1x1, with the fused tails, heads and pooling of its ConvExtra), k_conv1x1_chain_f16 (a bottleneck's conv3
// with the next block's conv1 chained), their filter packer and the pyramid-packed launches.  The deformable / AlignConv
// kernels these grew out of live in dcn_ops.hip; mfma_common.hpp holds what the two share.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "mfma_common.hpp"

namespace s2a {
namespace {

// weight [O][C][9] f16 -> [stage = cc*9+t][och group of 64][mt 2][kk 4][lane 64][8 halfs]:
// lane l, element j of fragment (mt,kk) = W[g*64 + mt*32 + (l&31)][cc*64 + kk*16 + 8*(l>>5) + j][t]
__global__ void k_pack_weight_frag(const _Float16* __restrict__ w, int O, int C, _Float16* __restrict__ wp,
                                   int taps = 9) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)O * C * taps;
  if (e >= total) return;
  const int G = O / 64;
  int j = (int)(e & 7);
  int lane = (int)((e >> 3) & 63);
  int kk = (int)((e >> 9) & 3);
  int mt = (int)((e >> 11) & 1);
  int64_t r = e >> 12;
  int g = (int)(r % G);
  int st = (int)(r / G);
  int t = st % taps, cc = st / taps;
  int och = g * 64 + mt * 32 + (lane & 31);
  int k = cc * 64 + kk * 16 + 8 * (lane >> 5) + j;
  wp[e] = w[((int64_t)och * C + k) * taps + t];
}

// ------------------------------------------------------------------ regular convolutions (f16)
// The conv towers of S2ANetHead (models/head.py:163-222: fam_reg_ls, fam_cls_ls, odm_reg_ls,
// odm_cls_ls, or_conv — nine 256->256 3x3 convolutions per FPN level) are the patch-staged
// AlignConv with integer sampling points: no blend, no column tile — the MFMA waves read their B
// fragments straight out of the LDS patch, the weights come in fragment order from L2, and a
// barrier is only needed once per 64-channel chunk.  256 threads = 4 waves; <= 67.6 KB of LDS ->
// two workgroups per CU, so one tile's prologue/epilogue overlaps the other's MFMA loop.  Bias,
// residual and ReLU are fused into the LDS-staged epilogue (one pass over the output instead of
// conv + bias/add/ReLU kernels).  TAPS = 9: 3x3/stride 1/pad 1 on an 8x16 position tile with a
// one-pixel halo.  TAPS = 1: 1x1 (stride 1 or 2) on 128 consecutive output positions — a plain
// GEMM with the same pipeline (the bottleneck 1x1 layers and FPN laterals of the carrier).
// OG = 64-channel output groups per workgroup (4, 2 or 1): with fewer than four groups the waves
// split the 128 positions instead, so narrow layers still use all four MFMA waves.
constexpr int kCPW = 18;                                  // stride 1: 16 positions + 1 halo each side

// PH = 128-position blocks per workgroup (1: 8 x 16 tile, 256 threads, two workgroups per CU; 2: 16 x 16 tile,
// 512 threads, one workgroup per CU, filter through LDS -- the pyramid-packed 256 -> 256 towers)
// optional second results computed from the staged output tile in the epilogue
struct ConvExtra {
  _Float16* pool_out;          // [P, O/8]: max over runs of 8 channels (rotation-invariant pooling) or null
  const _Float16* head_w;      // 1x1 prediction head on the tile: fragment-order filter (<= 32 maps, zero-padded) or null
  const _Float16* head_b;      // its bias (>= 32 entries)
  _Float16* head_out;          // [P, 64] (columns 0..31 written)
  int store_main;              // 0: the tower's own output is not needed (only the head reads it)
  // TAIL kernels only: the 1x1 convolution that follows (a bottleneck's conv3, models/backbone.py:60-83) applied to
  // the staged tile: out2 = relu(W2 . relu(conv + bias) + bias2 + residual2), 256 maps
  const _Float16* tail_w;      // fragment-order 1x1 filter [256][64]
  const _Float16* tail_b;      // [256]
  const _Float16* tail_res;    // [P, 256] or null
  _Float16* tail_out;          // [P, 256]
  // ... and optionally the NEXT bottleneck's conv1 (1x1, 256 -> 64, + bias + ReLU) on the finished output tile
  const _Float16* chain_w;     // fragment-order 1x1 filter [chain_O][256] or null
  const _Float16* chain_b;     // [chain_O]
  _Float16* chain_out;         // [P, chain_O]
  int chain_O;                 // 64 | 128
};

// SD = spatial stride of the 3x3 form (1, or 2: the down-sampling conv2 of a stage's first bottleneck; output tile
// 4 x 16 positions from a 9 x 33-pixel patch, two 32-position tiles per wave)
// HT = 1: 4 x 16 tile of a stride-1 3x3 (64 positions) for maps so small that 8 x 16 tiles leave CUs idle or give every
// CU a single workgroup (one wave per SIMD: nothing covers the weight / patch round trips)
template <int TAPS, int OG, int PH = 1, int SD = 1, bool TAIL = false, int HT = 0>
struct ConvCfg {
  static constexpr int kTH = (SD == 2 || HT) ? 4 : 8 * PH;             // tile rows (TAPS 9)
  static constexpr int kPos = (SD == 2 || HT) ? 64 : 128 * PH;         // output positions per workgroup
  static constexpr int kWaves = 4 * PH;
  static constexpr int kPW = SD == 2 ? 33 : kCPW;                      // patch width in pixels
  static constexpr int kNT = (kPos / 32) * OG / 4 / PH;                // 32-position tiles per wave
  static constexpr int kPix = TAPS == 9 ? ((kTH - 1) * SD + 3) * kPW : kPos;   // patch pixels
  static constexpr int kDma = (kPix * 9 + 63) / 64;                   // 1 KB LDS-DMA pieces per patch
  static constexpr int kPatchBytes = kDma * 1024;
  static constexpr int kOutRowB = OG * 128 + 16;                      // staged output row (bytes)
  // PH = 2 (TAPS 9, OG 4): the filter of a tap (32 KB) is staged through LDS once per workgroup, two buffers
  static constexpr bool kWLds = PH == 2 && TAPS == 9;
  static constexpr int kWBuf = OG * 8192;
  static constexpr int kLoop0 = 2 * kPatchBytes + (kWLds ? 2 * kWBuf : 0);
  // (OG 1 with the filter through LDS: room for all nine taps behind the first patch buffer)
  static constexpr int kLoop = (kWLds && OG == 1 && kPatchBytes + 9 * 8192 > kLoop0) ? kPatchBytes + 9 * 8192 : kLoop0;
  static constexpr int kLds0 = (kLoop > kPos * kOutRowB) ? kLoop : kPos * kOutRowB;
  static constexpr int kTailRowB = 528;                                // staged 256-map row of the fused 1x1
  static constexpr int kLds = (TAIL && kPos * kTailRowB > kLds0) ? kPos * kTailRowB : kLds0;
  static constexpr int kBiasBytes = TAIL ? 1024 : 512;
  static constexpr int kJ = (kDma + kWaves - 1) / kWaves;             // DMA pieces per wave
};

template <int TAPS, int OG, int PH = 1, int SD = 1, bool TAIL = false, int HT = 0>
__global__ __launch_bounds__(256 * PH, PH == 1 ? 2 : 1) void k_conv_f16(const _Float16* __restrict__ x_,
                                                     const _Float16* __restrict__ wfrag,
                                                     const _Float16* __restrict__ bias,
                                                     const _Float16* __restrict__ residual_,
                                                     _Float16* __restrict__ out_, int64_t Ntot_, int C,
                                                     int H_, int W_, int Ho_, int Wo_, int cstride, int O,
                                                     int relu, unsigned x_bytes_, LevelTab lt, int res_up,
                                                     ConvExtra ex) {
  _Float16* pool_out_ = ex.pool_out;
  using T = _Float16;
  using V = f16x8;
  using Cfg = ConvCfg<TAPS, OG, PH, SD, TAIL, HT>;
  constexpr int NT = Cfg::kNT;        // 32-position tiles per wave
  static_assert(NT >= 1, "unsupported tile / group combination");
  static_assert(!HT || (TAPS == 9 && PH == 1 && SD == 1 && !TAIL), "half tiles: plain 3x3 / stride 1");
  static_assert(!TAIL || (TAPS == 9 && OG == 1 && SD == 1), "the fused 1x1 tail follows a 64-map 3x3/s1");
  constexpr int WPG = 4 / OG;         // waves per out-channel group (inside a 128-position block)
  constexpr int kThreads_ = 256 * PH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave4 = wave & 3, blk = wave >> 2;     // wave inside its 128-position block, block index
  int64_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const T* x = x_;
  const T* residual = residual_;
  T* out = out_;
  int64_t Ntot = Ntot_;
  int H = H_, W = W_, Ho = Ho_, Wo = Wo_;
  unsigned x_bytes = x_bytes_;
  if (TAPS == 9 && lt.n > 1) {        // pyramid-packed levels: rebind this workgroup to its level
    int t0 = 0, p0 = 0;
#pragma unroll
    for (int i = 0; i < kMaxLevels; i++)
      if (i < lt.n && tile >= lt.tile0[i]) {
        t0 = lt.tile0[i]; p0 = lt.pix0[i]; H = lt.H[i]; W = lt.W[i];
      }
    tile -= t0;
    Ho = H; Wo = W;
    Ntot = (int64_t)lt.batch * H * W;
    x += (int64_t)p0 * C;
    out += (int64_t)p0 * O;
    if (residual) residual += (int64_t)p0 * O;
    if (pool_out_) pool_out_ += (int64_t)p0 * (O / 8);
    if (ex.head_out) ex.head_out += (int64_t)p0 * 64;
    x_bytes = (unsigned)(Ntot * C * 2);
  }
  const int64_t HWo = (int64_t)Ho * Wo, HWi = (int64_t)H * W;
  // TAPS 9: 2-D tile of one image; TAPS 1: 128 consecutive output positions of the whole batch
  const int txn = (Wo + 15) / 16, tyn = (Ho + Cfg::kTH - 1) / Cfg::kTH;
  const int64_t bimg = TAPS == 9 ? tile / (txn * tyn) : 0;
  const int trem = TAPS == 9 ? (int)(tile % (txn * tyn)) : 0;
  const int ty0 = (trem / txn) * Cfg::kTH, tx0 = (trem % txn) * 16;
  const int64_t g0 = tile * Cfg::kPos;
  const int o0 = blockIdx.y * (64 * OG);
  const int Oloc = min(64 * OG, O - o0);
  const int CC = (C + 63) / 64, G = O / 64;
  const int qlim = C >= 64 ? 8 : C / 8;   // C = 32: half-filled chunk, the filter is zero-padded to 64 inputs
  const unsigned row_bytes = (unsigned)C * 2;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, (int)x_bytes, 0x00020000);

  // Patch: global -> LDS by LDS-DMA (buffer_load ... lds).  One wave instruction writes 64 x 16 B
  // linearly; pixels sit 144 B apart (128 B of channels + a 16-byte pad chunk: conflict-free
  // ds_read_b128 fragments), linear slot v = pixel*9 + chunk; pad chunks and pixels outside the
  // image read an out-of-range offset (-> zeros).
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  unsigned pvoff[Cfg::kJ];
#pragma unroll
  for (int j = 0; j < Cfg::kJ; j++) {
    int v = (wave_u + Cfg::kWaves * j) * 64 + lane, p = v / 9, q = v % 9;
    bool in = q < qlim && p < Cfg::kPix;
    int64_t pix = 0;
    if (TAPS == 9) {
      int yy = ty0 * SD - 1 + p / Cfg::kPW, xx = tx0 * SD - 1 + p % Cfg::kPW;
      in = in && yy >= 0 && yy < H && xx >= 0 && xx < W;
      pix = bimg * HWi + (int64_t)yy * W + xx;
    } else {
      int64_t g = g0 + p;
      in = in && g < Ntot;
      int64_t bb = g / HWo, r = g % HWo;
      pix = bb * HWi + (r / Wo) * cstride * (int64_t)W + (r % Wo) * cstride;
    }
    pvoff[j] = in ? (unsigned)(pix * row_bytes + q * 16) : 0x80000000u;
  }
  // bias of this workgroup's out channels -> LDS (behind the tile buffers): the epilogue reads it
  // with ds_read instead of eight dependent global loads
  T* s_bias = reinterpret_cast<T*>(smem + Cfg::kLds);
  T bias_v = (T)0.f;
  if (bias && tid < Oloc) bias_v = bias[o0 + tid];   // in flight with the first patch / weights
  T tail_bias_v = (T)0.f;
  V wt[2][4];                                        // TAIL: this wave's 64 x 64 block of the 1x1 filter
  if constexpr (TAIL) {
    if (tid < 256) tail_bias_v = ex.tail_b[tid];
    // 16x16x32 fragments (f = 16-channel tile * 2 + k-step), as the stand-alone 1x1 takes them
    const V* tp = reinterpret_cast<const V*>(ex.tail_w) + (int64_t)wave4 * 8 * 64 + ((lane >> 4) & 1) * 128 + (lane >> 5) * 32 + (lane & 15);
#pragma unroll
    for (int f = 0; f < 8; f++) wt[f >> 2][f & 3] = tp[((f >> 2) * 4 + (f & 1)) * 64 + ((f >> 1) & 1) * 16];
  }
  auto patch_issue = [&](int cc) {
    char* P = smem + (cc & 1) * Cfg::kPatchBytes;
#pragma unroll
    for (int j = 0; j < Cfg::kJ; j++) {
      const int i = wave_u + Cfg::kWaves * j;
      if (i < Cfg::kDma)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(P + i * 1024), 16,
                                                 (int)pvoff[j], cc * 128, 0, 0);
    }
  };

  const int grp = wave4 / WPG, sub = wave4 % WPG;     // out-channel group, position sub-range (inside the block)
  const bool wave_active = grp * 64 < Oloc;
  const int g = min(o0 / 64 + grp, G - 1);
  const V* wf_base = reinterpret_cast<const V*>(wfrag) + lane;
  V wA[2][4], wB[2][4];
  // (every stride-1 3x3 launch and the full-width 1x1 launches; the narrower 1x1 launches stay on 32x32x16, as the chained conv1 of
  // the fused tail, which must agree with them bit for bit)
  // v_mfma_f32_16x16x32_f16 there (same-box: towers -5 ... -7 %, every full-width layer +3 % end to end)
  constexpr bool M16 = (TAPS == 9 && SD == 1) || (TAPS == 1 && OG == 4);
  constexpr int NB16 = 2 * NT;        // 16-position tiles per wave (8; 4 on the 64-position tiles)
  auto load_w = [&](int s, V (&wv)[2][4]) {
    if constexpr (M16) {
      // 16x16x32 fragments out of the same packed filter (lane maps below): fragment f = (16-channel tile f >> 1, k-step f & 1)
      const V* p = reinterpret_cast<const V*>(wfrag) + ((int64_t)s * G + g) * 8 * 64 + ((lane >> 4) & 1) * 128 + (lane >> 5) * 32 + (lane & 15);
#pragma unroll
      for (int f = 0; f < 8; f++) wv[f >> 2][f & 3] = p[((f >> 2) * 4 + (f & 1)) * 64 + ((f >> 1) & 1) * 16];
      return;
    }
    const V* p = wf_base + ((int64_t)s * G + g) * 8 * 64;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int kk = 0; kk < 4; kk++) wv[a][kk] = p[(a * 4 + kk) * 64];
  };
  // per N-tile b: byte offset of this lane's position (tap (0,0)) and k-half inside the patch;
  // the rest of a fragment address is a compile-time immediate (tap, kk)
  // lane -> position inside a 32-position tile.  3x3 / stride 1: a tile is two patch rows of 16 pixels, 18 pixels =
  // 162 sixteen-byte slots apart; ds_read_b128 serves lanes {0-3,12-15,20-27} (and the three like groups) in one
  // cycle only if their slots differ mod 16, and the second row's x = 4..11 land 2 slots-classes off the first row's
  // -> every group was 2-way conflicted (SQ_LDS_BANK_CONFLICT = half of the LDS cycles).  Rotating the second
  // row's pixels by two lanes makes all sixteen classes distinct; the epilogue uses the same map.
  const int lp = (TAPS == 9 && SD == 1) ? ((lane & 16) | (((lane & 15) - ((lane >> 3) & 2)) & 15)) : (lane & 31);
  int fbase[NT];
#pragma unroll
  for (int b = 0; b < NT; b++) {
    int pl = 128 * blk + 32 * (sub * NT + b) + lp;
    int pix = TAPS == 9 ? SD * ((pl >> 4) * Cfg::kPW + (pl & 15)) : pl;
    fbase[b] = pix * kRowBytes + (lane >> 5) * 16;
  }
  // full-width layers (OG 4, 128 positions per wave): v_mfma_f32_16x16x32_f16 -- same flops per cycle and the same LDS reads
  // per flop as 32x32x16, but the chip holds a higher clock on it under load (MI355X_MICROARCH.md, clocks (7): measured here
  // 187 -> 173 us on the pyramid towers, same box); the wave's 64 x 128 outputs are 4 x 8 tiles of 16 out channels x 16
  // positions (3x3: one patch row of 16 pixels)
  f32x16 acc[2][NT];
  f32x4 acc16[M16 ? 4 : 1][M16 ? NB16 : 1];
  if constexpr (M16) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < NB16; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc16[a][b][r] = 0.f;
  } else {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < NT; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
  }
  // 16x16x32 lane maps.  Lane l = (i = l & 15, kg = l >> 4).  Its eight k-values are the channel group c(ks, kg) =
  // {0, 4, 1, 5}[kg] + 2 ks of the 64-channel chunk (any order works as long as A and B agree): within the lane groups a
  // ds_read_b128 serves per cycle ({0-3,12-15,20-27}, ...) the two k-groups present then sit 64 B = 4 sixteen-byte slots
  // apart, and with the pixel map pix16 (i in 4..11 -> pixels = 0,1 mod 4, the others -> 2,3 mod 4; pixel pitch 9 slots)
  // all sixteen slots of a group differ -- conflict-free B reads.  The A fragment comes out of the SAME packed filter as
  // the 32x32x16 form: (out channel o, channel group c) is the 16 B at ((o>>5)*4 + (c>>1))*1 KB + ((c&1)*32 + (o&31))*16.
  const int kg16 = lane >> 4, i16 = lane & 15;
  const int pix16 = (i16 >= 4 && i16 < 12) ? (((i16 - 4) >> 1) * 4 + (i16 & 1))
                                           : (((i16 & 3) >> 1) * 4 + 2 + (i16 & 1) + (i16 >= 12 ? 8 : 0));
  const int t16 = 2 * sub * NT;                   // first 16-position tile of this wave inside its 128-position block
  const int fbase16 = (TAPS == 9 ? (8 * blk + t16) * Cfg::kPW + pix16 : 128 * blk + 16 * t16 + pix16) * kRowBytes + (kg16 & 1) * 64 + (kg16 >> 1) * 16;
  constexpr int kTile16 = (TAPS == 9 ? Cfg::kPW : 16) * kRowBytes;      // LDS distance between a wave's 16-position tiles
  const int abase16 = (kg16 & 1) * 2048 + ((kg16 >> 1) * 32 + i16) * 16;

  auto compute = [&](const char* P, int t, const V (&wv)[2][4]) {
    if (!wave_active) return;
    const int toff = ((t / 3) * Cfg::kPW + (t % 3)) * kRowBytes;
    if constexpr (M16) {
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        V pf[NB16];
#pragma unroll
        for (int b = 0; b < NB16; b++) pf[b] = *reinterpret_cast<const V*>(P + fbase16 + b * kTile16 + toff + ks * 32);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < NB16; b++)
            acc16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[(a * 2 + ks) >> 2][(a * 2 + ks) & 3], pf[b], acc16[a][b], 0, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      V pf[NT];
#pragma unroll
      for (int b = 0; b < NT; b++) pf[b] = *reinterpret_cast<const V*>(P + fbase[b] + toff + kk * 32);
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < NT; b++)
          acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv[a][kk], pf[b], acc[a][b], 0, 0, 0);
    }
  };

  // fused tail: residual vectors of the whole 256-map tile.  With the filter through LDS (16 x 16 tiles) they are requested
  // right after the prologue's barrier: the 3x3 GEMM waits on LDS reads only, so the 128 KB are in flight under it and under
  // the first epilogue instead of in front of the second one (at kernel start they queue ahead of the patch and the
  // filter on the in-order memory path: measured slower).  Register-filter form: requested behind the second GEMM, as before.
  constexpr bool kEarlyRes = TAIL && Cfg::kWLds;
  constexpr int NI2 = TAIL ? Cfg::kPos * 32 / kThreads_ : 1;
  unsigned off2[NI2];
  V r2[NI2];
  auto tail_res_issue = [&]() {
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(ex.tail_res ? ex.tail_res : ex.tail_out), 0, (int)((uint64_t)Ntot * 256 * 2), 0x00020000);
#pragma unroll
    for (int i = 0; i < NI2; i++) {
      const int idx = tid + kThreads_ * i, pos = idx >> 5, col = idx & 31;
      const int64_t gp = tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot);
      off2[i] = gp >= 0 ? (unsigned)((gp * 256 + col * 8) * 2) : 0x80000000u;
      r2[i] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)(ex.tail_res ? off2[i] : 0x80000000u), 0, 0));
    }
  };
  const int nstage = TAPS * CC, last = nstage - 1;
  if constexpr (Cfg::kWLds) {
    // 16 x 16 tile, filter through LDS: every tap's 32 KB (this workgroup's 256 out channels, fragment order =
    // contiguous) is DMA-ed once into one of two LDS buffers while the previous tap computes; all eight waves
    // read their A fragments from there (ds_read_b128, lane-linear).  Halves the filter bytes a CU pulls per
    // flop compared with two 8 x 16 workgroups; costs a barrier per tap.
    char* wb = smem + 2 * Cfg::kPatchBytes;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(wfrag), 0, (int)((uint64_t)O * (uint64_t)(CC * 64) * 9 * 2), 0x00020000);
    const int wbase = (o0 / 64) * 8192;
    auto w_issue = [&](int s) {      // 8 * OG pieces of 1 KB over the eight waves
#pragma unroll
      for (int j = 0; j < OG; j++) {
        const int piece = wave_u * OG + j;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(wb + (s & 1) * Cfg::kWBuf + piece * 1024),
                                                 16, piece * 1024 + lane * 16, s * G * 8192 + wbase, 0, 0);
      }
    };
    auto compute_wl = [&](const char* P, int t, const char* Wb) {
      const int toff = ((t / 3) * Cfg::kPW + (t % 3)) * kRowBytes;
      if constexpr (M16) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
          V wv[4], pf[NB16];
#pragma unroll
          for (int a = 0; a < 4; a++)
            wv[a] = *reinterpret_cast<const V*>(Wb + grp * 8192 + abase16 + (a >> 1) * 4096 + ks * 1024 + (a & 1) * 256);
#pragma unroll
          for (int b = 0; b < NB16; b++)
            pf[b] = *reinterpret_cast<const V*>(P + fbase16 + b * kTile16 + toff + ks * 32);
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < NB16; b++)
              acc16[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[a], pf[b], acc16[a][b], 0, 0, 0);
        }
        return;
      }
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
        V pf[NT], wv[2];
#pragma unroll
        for (int a = 0; a < 2; a++) wv[a] = *reinterpret_cast<const V*>(Wb + (((grp * 2 + a) * 4 + kk) * 64 + lane) * 16);
#pragma unroll
        for (int b = 0; b < NT; b++) pf[b] = *reinterpret_cast<const V*>(P + fbase[b] + toff + kk * 32);
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < NT; b++)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wv[a], pf[b], acc[a][b], 0, 0, 0);
      }
    };
    if (OG == 1 && CC == 1) {
      // 64 input maps, one out-channel group: the WHOLE 3x3 filter (9 x 8 KB) goes into LDS at once (over the second
      // patch buffer, which a one-chunk layer never uses) -- one memory latency per tile instead of one per tap
      // (eight MFMAs per wave and tap cannot cover an L2 round trip), and no barrier inside the tile
      char* wall = smem + Cfg::kPatchBytes;
      patch_issue(0);
#pragma unroll
      for (int t = 0; t < 9; t++)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(wall + t * 8192 + wave_u * 1024),
                                                 16, wave_u * 1024 + lane * 16, t * G * 8192 + wbase, 0, 0);
      if (tid < 64) s_bias[tid] = bias_v;
      if constexpr (TAIL) { if (tid < 256) s_bias[64 + tid] = tail_bias_v; }
      __syncthreads();
      if constexpr (kEarlyRes) tail_res_issue();
#pragma unroll
      for (int t = 0; t < 9; t++) compute_wl(smem, t, wall + t * 8192);
      __syncthreads();
    } else {
    patch_issue(0);
    w_issue(0);
    if (tid < 64 * OG) s_bias[tid] = bias_v;
    if constexpr (TAIL) { if (tid < 256) s_bias[64 + tid] = tail_bias_v; }
    __syncthreads();
    // (Measured dead end, round 2: fragments one k-step ahead in two register sets across taps, the barrier in front of
    // the tap's last k-step with counted vmcnt, DMAs issued behind it -- bit-identical and within noise of this form,
    // 219-225 vs 222 us: at two waves per SIMD the partner wave already covers these waits.  Timing-only ablations of
    // that form: no filter DMA in the loop -7 %, no patch DMA 0 %, no barrier -3 %, neither -11 %.)
    for (int cc = 0; cc < CC; cc++) {
      const char* Pc = smem + (cc & 1) * Cfg::kPatchBytes;
#pragma unroll
      for (int t = 0; t < 9; t++) {
        const int s = cc * 9 + t;
        if (s + 1 < nstage) w_issue(s + 1);
        if (t == 0 && cc + 1 < CC) patch_issue(cc + 1);
        compute_wl(Pc, t, wb + (s & 1) * Cfg::kWBuf);
        __syncthreads();     // drains this tap's DMAs (vmcnt(0)) and frees the buffers they will overwrite next
      }
    }
    }
  } else {
  patch_issue(0);
  load_w(0, wA);
  if (tid < 64 * OG) s_bias[tid] = bias_v;
  if constexpr (TAIL) { if (tid < 256) s_bias[64 + tid] = tail_bias_v; }
  __syncthreads();   // (the compiler drains the DMA with vmcnt(0) before the barrier)
  if constexpr (TAPS == 9) {
    for (int cc = 0; cc < CC; cc++) {
      const int s0 = cc * 9;
      const char* Pc = smem + (cc & 1) * Cfg::kPatchBytes;
      // 9 taps, weight fragments double-buffered in registers (static indexing: unrolled by hand)
#define S2A_TAP(T_, WCUR, WNEXT)                                                     \
      load_w(min(s0 + (T_) + 1, last), WNEXT);                                          \
      compute(Pc, (T_), WCUR);                                                          \
      __builtin_amdgcn_sched_barrier(0); /* keep the next taps' loads from being hoisted (registers) */
      S2A_TAP(0, wA, wB)
      S2A_TAP(1, wB, wA)
      S2A_TAP(2, wA, wB)
      S2A_TAP(3, wB, wA)
      S2A_TAP(4, wA, wB)
      S2A_TAP(5, wB, wA)
      // next chunk's patch: issued here so that tap 6 still runs on weights loaded before the DMA
      // (vmcnt is in-order) and taps 6-8 cover its latency
      if (cc + 1 < CC) patch_issue(cc + 1);
      S2A_TAP(6, wA, wB)
      S2A_TAP(7, wB, wA)
      S2A_TAP(8, wA, wB)
#undef S2A_TAP
      __syncthreads();
      // after an odd number of taps the roles of wA/wB are swapped: copy back (8 v_movs per chunk)
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) wA[a][kk] = wB[a][kk];
    }
  } else {
    // one stage per 64-channel chunk: next chunk's tile and weights in flight under this one's MFMAs
#define S2A_STAGE(C_, WCUR, WNEXT)                                                   \
    if ((C_) + 1 < CC) patch_issue((C_) + 1);                                           \
    load_w(min((C_) + 1, last), WNEXT);                                                 \
    compute(smem + ((C_) & 1) * Cfg::kPatchBytes, 0, WCUR);                             \
    __syncthreads();
    int cc = 0;
    for (; cc + 1 < CC; cc += 2) {
      S2A_STAGE(cc, wA, wB)
      S2A_STAGE(cc + 1, wB, wA)
    }
    if (cc < CC) { S2A_STAGE(cc, wA, wB) }
#undef S2A_STAGE
  }
  }   // !kWLds

  // ---- epilogue: bias (+ residual) + ReLU; tile staged through LDS, rows stored 16 B per lane
  char* s_out = smem;
  // ReLU on the ROUNDED halves, two per instruction (rounding is monotonic and keeps zero: max(round(v), 0) == round(max(v, 0));
  // NaN -> 0 either way), and the ReLU switch as one uniform branch around the tile -- fmaxf plus a per-value select on the
  // f32 sums was 9 instructions per two values, 4.8 k of a tower tile's 113 k cycles (same-box A/B: pyramid tower launch
  // 195.9 -> 191.4 us on dense data)
  using h2e = __attribute__((ext_vector_type(2))) _Float16;
  using h4e = __attribute__((ext_vector_type(4))) _Float16;
  auto stage_tile = [&](auto relu_c) {
    constexpr bool kRelu = decltype(relu_c)::value;
    auto quad = [&](float v0, float v1, float v2, float v3, const h4e& bq) {
      h2e lo = {(_Float16)(v0 + (float)bq[0]), (_Float16)(v1 + (float)bq[1])};
      h2e hi = {(_Float16)(v2 + (float)bq[2]), (_Float16)(v3 + (float)bq[3])};
      if constexpr (kRelu) {
        lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
        hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
      }
      return h4e{lo[0], lo[1], hi[0], hi[1]};
    };
    if constexpr (M16) {
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const int och = grp * 64 + 16 * a + 4 * kg16;       // D: row (out channel) = 4 (lane >> 4) + register, column = pixel
        const h4e bq = *reinterpret_cast<const h4e*>(s_bias + och);
#pragma unroll
        for (int b = 0; b < NB16; b++) {
          const int pos = 128 * blk + 16 * (t16 + b) + pix16;
          *reinterpret_cast<h4e*>(s_out + pos * Cfg::kOutRowB + och * 2) =
              quad(acc16[a][b][0], acc16[a][b][1], acc16[a][b][2], acc16[a][b][3], bq);
        }
      }
    } else {
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int rq = 0; rq < 4; rq++) {
          const int och = grp * 64 + 32 * a + 8 * rq + 4 * (lane >> 5);
          const h4e bq = *reinterpret_cast<const h4e*>(s_bias + och);
#pragma unroll
          for (int b = 0; b < NT; b++) {
            int pos = 128 * blk + 32 * (sub * NT + b) + lp;
            *reinterpret_cast<h4e*>(s_out + pos * Cfg::kOutRowB + och * 2) =
                quad(acc[a][b][rq * 4], acc[a][b][rq * 4 + 1], acc[a][b][rq * 4 + 2], acc[a][b][rq * 4 + 3], bq);
          }
        }
    }
  };
  if (wave_active) {
    if (relu && !residual) stage_tile(std::true_type{}); else stage_tile(std::false_type{});
  }
  __syncthreads();
  if constexpr (TAIL) {
    // ---- fused 1x1 (64 -> 256) on the staged tile: wave w = out maps 64w..64w+63 x the 128 positions of its block,
    // B fragments from the staged rows (144-byte stride: conflict-free), accumulation order = the stand-alone 1x1's
    // (the second GEMM on 16x16x32 MFMAs, as the stand-alone 64 -> 256 1x1)
    f32x4 acc3s[4][8];
    {
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 8; b++)
#pragma unroll
          for (int r = 0; r < 4; r++) acc3s[a][b][r] = 0.f;
      const char* brow = s_out + (128 * blk + pix16) * Cfg::kOutRowB + (kg16 & 1) * 64 + (kg16 >> 1) * 16;
#pragma unroll
      for (int ks = 0; ks < 2; ks++)
#pragma unroll
        for (int bh = 0; bh < 8; bh += 4) {      // four position tiles at a time: the residual prefetch below needs the registers
          V pf[4];
#pragma unroll
          for (int b = 0; b < 4; b++) pf[b] = *reinterpret_cast<const V*>(brow + (bh + b) * 16 * Cfg::kOutRowB + ks * 32);
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++)
              acc3s[a][bh + b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[(a * 2 + ks) >> 2][(a * 2 + ks) & 3], pf[b], acc3s[a][bh + b], 0, 0, 0);
        }
    }
    // residual vectors of the whole tile in flight before the tile is re-staged (issuing them at kernel start was
    // slower: they queue ahead of the patch and the filters on the in-order memory path)
    if constexpr (!kEarlyRes) {
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<T*>(ex.tail_res ? ex.tail_res : ex.tail_out), 0, (int)((uint64_t)Ntot * 256 * 2), 0x00020000);
#pragma unroll
      for (int i = 0; i < NI2; i++) {
        const int idx = tid + kThreads_ * i, pos = idx >> 5, col = idx & 31;
        const int64_t gp = tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot);
        off2[i] = gp >= 0 ? (unsigned)((gp * 256 + col * 8) * 2) : 0x80000000u;
        r2[i] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)(ex.tail_res ? off2[i] : 0x80000000u), 0, 0));
      }
    }
    __syncthreads();                       // every wave has read its B fragments: the tile may be overwritten
    {
      using h4 = __attribute__((ext_vector_type(4))) _Float16;
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const int och = wave4 * 64 + 16 * a + 4 * kg16;
        const h4 bq = *reinterpret_cast<const h4*>(s_bias + 64 + och);
#pragma unroll
        for (int b = 0; b < 8; b++) {
          h4 v4;
#pragma unroll
          for (int e = 0; e < 4; e++) v4[e] = (_Float16)(acc3s[a][b][e] + (float)bq[e]);
          *reinterpret_cast<h4*>(s_out + (128 * blk + 16 * b + pix16) * Cfg::kTailRowB + och * 2) = v4;
        }
      }
    }
    __syncthreads();
    // chained conv1: its 16 filter fragments are requested here, in front of the residual add / store pass (they were
    // loaded behind it, one exposed L2 round trip per tile in front of the third GEMM)
    const int O3 = ex.chain_O, MT = max(O3 / 32, 1);                // 2 | 4 m-tiles
    const int nper = (Cfg::kPos / 32) * MT / Cfg::kWaves;          // 32-position tiles per wave: 2 | 4
    const int mt = wave % MT, nt0 = (wave / MT) * nper;
    const int G3 = O3 / 64;
    V aw[16];
    if (ex.chain_w) {
      const V* cwp = reinterpret_cast<const V*>(ex.chain_w) + lane + ((mt >> 1) * 8 + (mt & 1) * 4) * 64;
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) aw[c4 * 4 + kk] = cwp[(c4 * G3 * 8 + kk) * 64];
    }
#pragma unroll
    for (int i = 0; i < NI2; i++) {
      const int idx = tid + kThreads_ * i, pos = idx >> 5, col = idx & 31;
      V v = *reinterpret_cast<const V*>(s_out + pos * Cfg::kTailRowB + col * 16);
#pragma unroll
      for (int e = 0; e < 8; e += 2) {     // (ReLU on the rounded halves, two per instruction: see the epilogue above)
        h2e p2 = {(_Float16)((float)v[e] + (float)r2[i][e]), (_Float16)((float)v[e + 1] + (float)r2[i][e + 1])};
        p2 = __builtin_elementwise_max(p2, h2e{(_Float16)0.f, (_Float16)0.f});
        v[e] = p2[0];
        v[e + 1] = p2[1];
      }
      if (off2[i] != 0x80000000u) *reinterpret_cast<V*>(reinterpret_cast<char*>(ex.tail_out) + off2[i]) = v;
      if (ex.chain_w) *reinterpret_cast<V*>(s_out + pos * Cfg::kTailRowB + col * 16) = v;   // finished rows back to LDS
    }
    if (ex.chain_w) {
      // ---- the next block's conv1 on the finished 256-map tile: out3 = relu(W . y + b), 64 maps (same stage) or 128
      // (first block of the next stage).  wave = (m-tile, a run of 32-position tiles); B fragments from the staged
      // rows (528-byte stride: conflict-free), the 16 filter fragments of the m-tile straight from L2; K order =
      // the stand-alone 1x1 kernel's (chunk, k-step).
      f32x16 c2[4];
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) c2[j][r] = 0.f;
      __syncthreads();                     // the whole finished tile is in LDS
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++)
#pragma unroll
          for (int j = 0; j < 4; j++)
            if (j < nper) {
              const V bf = *reinterpret_cast<const V*>(s_out + (32 * (nt0 + j) + (lane & 31)) * Cfg::kTailRowB +
                                                       (c4 * 64 + kk * 16 + (lane >> 5) * 8) * 2);
              c2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aw[c4 * 4 + kk], bf, c2[j], 0, 0, 0);
            }
      __syncthreads();                     // every wave has read its B fragments: the tile area is free again
      // tile -> LDS rows (O3 * 2 + 16 bytes) -> whole rows stored 16 B per lane (8-byte stores straight from the MFMA
      // layout cost more than the GEMM)
      const int rowb = O3 * 2 + 16;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j < nper) {
#pragma unroll
          for (int rq = 0; rq < 4; rq++) {
            using h4 = __attribute__((ext_vector_type(4))) _Float16;
            const int och = mt * 32 + 8 * rq + 4 * (lane >> 5);
            const h4 bq = *reinterpret_cast<const h4*>(ex.chain_b + och);
            h2e lo = {(_Float16)(c2[j][rq * 4] + (float)bq[0]), (_Float16)(c2[j][rq * 4 + 1] + (float)bq[1])};
            h2e hi = {(_Float16)(c2[j][rq * 4 + 2] + (float)bq[2]), (_Float16)(c2[j][rq * 4 + 3] + (float)bq[3])};
            lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
            hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
            const h4 v4 = {lo[0], lo[1], hi[0], hi[1]};
            *reinterpret_cast<h4*>(s_out + (32 * (nt0 + j) + (lane & 31)) * rowb + och * 2) = v4;
          }
        }
      __syncthreads();
      const int vpr = O3 / 8;                                          // 16-byte vectors per row: 8 | 16
      for (int idx = tid; idx < Cfg::kPos * vpr; idx += kThreads_) {
        const int pos = idx / vpr, col = idx % vpr;
        const int64_t gp = tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot);
        if (gp >= 0)
          *reinterpret_cast<V*>(ex.chain_out + gp * O3 + col * 8) = *reinterpret_cast<const V*>(s_out + pos * rowb + col * 16);
      }
    }
    return;
  }
  constexpr int VPR = 8 * OG;                     // 16-byte vectors per output row
  constexpr int NI = (Cfg::kPos * VPR) / kThreads_;
  const bool relu_u = __builtin_amdgcn_readfirstlane(relu) != 0;
  if (residual) {
    // all residual vectors of the tile in flight at once (bounds-checked buffer loads: no branch
    // around a load, so the compiler does not wait for each one before issuing the next)
    // res_up: the residual is a half-resolution map [B,Ho/2,Wo/2,O] added through a nearest 2x
    // up-sampling (the FPN top-down pathway, models/neck.py:73-79) -- only its row index differs
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<T*>(residual), 0, (int)((uint64_t)(res_up ? Ntot / 4 : Ntot) * O * 2), 0x00020000);
    unsigned off[NI];
    V r[NI];
    const int Wr = Wo >> 1;
    const int64_t HWr = (int64_t)(Ho >> 1) * Wr;
#pragma unroll
    for (int i = 0; i < NI; i++) {
      int idx = tid + kThreads_ * i, pos = idx / VPR, col = idx % VPR;
      int64_t gp = TAPS == 9 ? tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot) : (g0 + pos < Ntot ? g0 + pos : -1);
      const bool ok = gp >= 0 && col * 8 < Oloc;
      off[i] = ok ? (unsigned)((gp * O + o0 + col * 8) * 2) : 0x80000000u;
      unsigned roff = off[i];
      if (res_up && ok) {
        const int64_t bb = gp / HWo, rem = gp % HWo;
        const int yy = (int)(rem / Wo), xx = (int)(rem % Wo);
        roff = (unsigned)(((bb * HWr + (int64_t)(yy >> 1) * Wr + (xx >> 1)) * O + o0 + col * 8) * 2);
      }
      r[i] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rr, (int)roff, 0, 0));
    }
#pragma unroll
    for (int i = 0; i < NI; i++) {
      int idx = tid + kThreads_ * i, pos = idx / VPR, col = idx % VPR;
      V v = *reinterpret_cast<const V*>(s_out + pos * Cfg::kOutRowB + col * 16);
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        h2e p2 = {(_Float16)((float)v[e] + (float)r[i][e]), (_Float16)((float)v[e + 1] + (float)r[i][e + 1])};
        if (relu_u) p2 = __builtin_elementwise_max(p2, h2e{(_Float16)0.f, (_Float16)0.f});   // (on the rounded halves: see above)
        v[e] = p2[0];
        v[e + 1] = p2[1];
      }
      if (off[i] != 0x80000000u) *reinterpret_cast<V*>(reinterpret_cast<char*>(out) + off[i]) = v;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      int idx = tid + kThreads_ * i, pos = idx / VPR, col = idx % VPR;
      int64_t gp = TAPS == 9 ? tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot) : (g0 + pos < Ntot ? g0 + pos : -1);
      if (gp >= 0 && col * 8 < Oloc && ex.store_main)
        *reinterpret_cast<V*>(out + gp * O + o0 + col * 8) = *reinterpret_cast<const V*>(s_out + pos * Cfg::kOutRowB + col * 16);
    }
  }
  // optional: a 1x1 prediction head (<= 32 maps: fam_reg_head / fam_cls_head, models/head.py:205-213) applied to
  // the staged tile -- every wave takes 32 positions, B fragments straight from the staged rows (528-byte stride:
  // conflict-free), A fragments = the head's filter (16 KB, L2-resident), 16 MFMAs.  Needs the whole channel range
  // in this workgroup (OG = 4, O = 256).
  if constexpr (OG == 4) {
    if (ex.head_w) {
      f32x16 hacc;
#pragma unroll
      for (int r = 0; r < 16; r++) hacc[r] = 0.f;
      const int hpos = 32 * wave + (lane & 31);
      const V* hw = reinterpret_cast<const V*>(ex.head_w) + lane;
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          const V a = hw[(c4 * 8 + kk) * 64];                 // stage c4, m-tile 0 (maps 0..31), k-step kk
          const V b = *reinterpret_cast<const V*>(s_out + hpos * Cfg::kOutRowB + (c4 * 64 + kk * 16 + (lane >> 5) * 8) * 2);
          hacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, hacc, 0, 0, 0);
        }
      const int64_t gp = TAPS == 9 ? tile_pos(tile, hpos, Cfg::kTH, Ho, Wo, HWo, Ntot) : (g0 + hpos < Ntot ? g0 + hpos : -1);
      if (gp >= 0) {
        using h4 = __attribute__((ext_vector_type(4))) _Float16;
#pragma unroll
        for (int rq = 0; rq < 4; rq++) {
          const int och = 8 * rq + 4 * (lane >> 5);
          const h4 hb = *reinterpret_cast<const h4*>(ex.head_b + och);
          h4 v4;
#pragma unroll
          for (int e = 0; e < 4; e++) v4[e] = (_Float16)(hacc[rq * 4 + e] + (float)hb[e]);
          *reinterpret_cast<h4*>(ex.head_out + gp * 64 + och) = v4;
        }
      }
    }
  }
  // optional second output: rotation-invariant pooling of the tile just produced (max over each run of 8
  // orientation channels, models/orn/functions/rotation_invariant_pooling.py:19-27) straight from the staged
  // tile -- ORConv2d's output feeds both the regression tower (full tile, stored above) and, pooled, the
  // classification tower.  One item = one position x 8 pooled channels (128 B read, 16 B stored).
  if (pool_out_) {
    constexpr int GP = 8 * OG;                      // pooled channels of this workgroup's 64*OG outputs
    for (int item = tid; item < Cfg::kPos * (GP / 8); item += kThreads_) {
      const int pos = item / (GP / 8), q = item % (GP / 8);
      const int64_t gp = TAPS == 9 ? tile_pos(tile, pos, Cfg::kTH, Ho, Wo, HWo, Ntot) : (g0 + pos < Ntot ? g0 + pos : -1);
      if (gp < 0 || q * 64 >= Oloc) continue;
      V res;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const V v = *reinterpret_cast<const V*>(s_out + pos * Cfg::kOutRowB + (q * 8 + e) * 16);
        _Float16 mx = v[0];
#pragma unroll
        for (int k = 1; k < 8; k++) mx = v[k] > mx ? v[k] : mx;
        res[e] = mx;
      }
      *reinterpret_cast<V*>(pool_out_ + gp * (O / 8) + o0 / 8 + q * 8) = res;
    }
  }
}

// ------------------------------------------------------------------ 1x1 + residual + ReLU with the next block's conv1 chained
// A bottleneck's conv3 (1x1, K -> O = 4 K, + bias + residual + ReLU, models/backbone.py:69-83) and the NEXT bottleneck's
// conv1 (1x1, O -> O3, + bias + ReLU) in one launch: the block output is written once and not read back by a second
// launch.  A workgroup (4 waves, 64 consecutive positions) owns ALL O channels of its positions: the input tile (K <= 256:
// up to four 64-channel chunks at the 144-byte pixel pitch) stays in LDS, and the 256-map output groups are walked one
// after the other -- GEMM (wave = 64 maps x 64 positions), rows staged through LDS (528-byte pitch), residual + ReLU,
// whole-row stores, finished rows back to LDS, then this group's 256-channel K-slice of the chained GEMM into accumulators
// that live across the groups.  <= 72 KB of LDS and <= 256 registers: two workgroups per CU, one's memory passes under the
// other's MFMAs.
// Both results are bit-identical to the stand-alone launches of k_conv_f16: the main GEMM and a chained layer of 256 / 512
// maps use its 16x16x32 fragments (the full-width 1x1 form), a chained layer of 128 maps its 32x32x16 form (OG = 2); the
// accumulation order over the input channels is ascending in both, and the epilogue roundings are the same
// (rnd16(rnd16(acc + b) + r), ReLU on the rounded halves).
template <int CC, int O3>
__global__ __launch_bounds__(256, 2) void k_conv1x1_chain_f16(const _Float16* __restrict__ x,
                                                              const _Float16* __restrict__ wfrag,
                                                              const _Float16* __restrict__ bias,
                                                              const _Float16* __restrict__ residual,
                                                              _Float16* __restrict__ out,
                                                              const _Float16* __restrict__ chain_w,
                                                              const _Float16* __restrict__ chain_b,
                                                              _Float16* __restrict__ chain_out, int64_t Ntot,
                                                              unsigned x_bytes) {
  using T = _Float16;
  using V = f16x8;
  using h2e = __attribute__((ext_vector_type(2))) _Float16;
  using h4e = __attribute__((ext_vector_type(4))) _Float16;
  constexpr int kPos = 64, kChunkB = kPos * kRowBytes, kStRowB = 528;
  constexpr bool C16 = O3 >= 256;               // chained layer on 16x16x32 fragments (stand-alone: OG = 4)
  constexpr int NG3 = C16 ? O3 / 256 : 1;       // 64-map groups of the chained layer per wave
  constexpr int G3 = O3 / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int64_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t g0 = tile * kPos;
  constexpr int K = 64 * CC, O = 4 * K, NG = O / 256, G = O / 64;     // (a bottleneck's conv3: O = 4 K)
  char* s_x = smem;
  char* s_st = smem + CC * kChunkB;
  T* s_bias = reinterpret_cast<T*>(s_st + kPos * kStRowB);

  // input tile -> LDS by LDS-DMA, every chunk at once (layout and zero fill: k_conv_f16's TAPS = 1 patch)
  {
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, (int)x_bytes, 0x00020000);
    unsigned pvoff[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int v = (wave_u + 4 * j) * 64 + lane, p = v / 9, q = v % 9;
      const bool in = q < 8 && p < kPos && g0 + p < Ntot;
      pvoff[j] = in ? (unsigned)((g0 + p) * K * 2 + q * 16) : 0x80000000u;
    }
#pragma unroll
    for (int cc = 0; cc < CC; cc++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int i = wave_u + 4 * j;
        if (i < 9)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(s_x + cc * kChunkB + i * 1024), 16,
                                                   (int)pvoff[j], cc * 128, 0, 0);
      }
  }

  // 16x16x32 lane maps and fragment addresses: k_conv_f16
  const int kg16 = lane >> 4, i16 = lane & 15;
  const int pix16 = (i16 >= 4 && i16 < 12) ? (((i16 - 4) >> 1) * 4 + (i16 & 1))
                                           : (((i16 & 3) >> 1) * 4 + 2 + (i16 & 1) + (i16 >= 12 ? 8 : 0));
  const int bofs = (kg16 & 1) * 64 + (kg16 >> 1) * 16;
  const int wlane = ((lane >> 4) & 1) * 128 + (lane >> 5) * 32 + (lane & 15);
  // filter fragments one k-step (half a 64-channel chunk) at a time: the four 16-map tiles of group g, stage s
  auto load_w16 = [&](const T* wf, int s, int Gn, int g, int ks, V (&wv)[4]) {
    const V* p = reinterpret_cast<const V*>(wf) + ((int64_t)s * Gn + g) * 8 * 64 + wlane + ks * 64;
#pragma unroll
    for (int a = 0; a < 4; a++) wv[a] = p[(a >> 1) * 4 * 64 + (a & 1) * 16];
  };
  // one k-step: 64 maps x 64 positions of this wave; brow = the lane's B row of the first 16-position tile
  auto mma16 = [&](const char* brow, int tile_b, int ks, const V (&wv)[4], f32x4 (&acc)[4][4]) {
    V pf[4];
#pragma unroll
    for (int b = 0; b < 4; b++) pf[b] = *reinterpret_cast<const V*>(brow + b * tile_b + ks * 32);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[a], pf[b], acc[a][b], 0, 0, 0);
  };

  // accumulators of the chained layer, live across the output groups
  f32x4 cacc[C16 ? NG3 : 1][4][4];
  f32x16 c2[2];
  if constexpr (C16) {
#pragma unroll
    for (int n = 0; n < NG3; n++)
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
          for (int r = 0; r < 4; r++) cacc[n][a][b][r] = 0.f;
  } else {
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) c2[j][r] = 0.f;
  }
  const bool has_res = residual != nullptr;
  const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(has_res ? residual : out), 0,
                                                                      (int)((uint64_t)Ntot * O * 2), 0x00020000);
  const int pos0 = tid >> 5, col0 = tid & 31;
  const int nvalid = (int)(Ntot - g0 < kPos ? Ntot - g0 : kPos);     // positions of this tile inside the batch
  const unsigned off0 = (unsigned)(((g0 + pos0) * O + col0 * 8) * 2);
  __syncthreads();   // the input tile is in LDS (the DMA is drained in front of the barrier)

#pragma unroll 1
  for (int gi = 0; gi < NG; gi++) {
    const int o0 = gi * 256;
    s_bias[tid] = bias[o0 + tid];      // read behind the next barrier
    // ---- main GEMM of this group
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) acc[a][b][r] = 0.f;
    {
      V w[2][4];
      load_w16(wfrag, 0, G, gi * 4 + wave, 0, w[0]);
#pragma unroll
      for (int st = 0; st < 2 * CC; st++) {
        if (st + 1 < 2 * CC) load_w16(wfrag, (st + 1) >> 1, G, gi * 4 + wave, (st + 1) & 1, w[(st + 1) & 1]);
        mma16(s_x + (st >> 1) * kChunkB + pix16 * kRowBytes + bofs, 16 * kRowBytes, st & 1, w[st & 1], acc);
        __builtin_amdgcn_sched_barrier(0);   // keep the later k-steps' loads from being hoisted (registers)
      }
    }
    // residual vectors of the group's tile in flight under the staging
    // (vector i of a thread: position pos0 + 8 i, 16-byte column col0 -- rows 8 positions = 8 * O * 2 bytes apart)
    const unsigned offg = off0 + o0 * 2;
    V r8[8];
    if (has_res) {
#pragma unroll
      for (int i = 0; i < 8; i++)
        r8[i] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(
                                          rr, (int)(pos0 + 8 * i < nvalid ? offg + i * (8 * O * 2) : 0x80000000u), 0, 0));
    }
    __syncthreads();   // the previous group's chained GEMM has read the staged rows; s_bias is written
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int och = wave * 64 + 16 * a + 4 * kg16;
      const h4e bq = *reinterpret_cast<const h4e*>(s_bias + och);
#pragma unroll
      for (int b = 0; b < 4; b++) {
        h2e lo = {(_Float16)(acc[a][b][0] + (float)bq[0]), (_Float16)(acc[a][b][1] + (float)bq[1])};
        h2e hi = {(_Float16)(acc[a][b][2] + (float)bq[2]), (_Float16)(acc[a][b][3] + (float)bq[3])};
        if (!has_res) {
          lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
          hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
        }
        *reinterpret_cast<h4e*>(s_st + (16 * b + pix16) * kStRowB + och * 2) = h4e{lo[0], lo[1], hi[0], hi[1]};
      }
    }
    __syncthreads();
    // chained filter fragments requested in front of the residual / store pass
    V aw[C16 ? 4 : 16];
    if constexpr (C16) {
      load_w16(chain_w, gi * 4, G3, wave, 0, aw);
    } else {
      const V* cwp = reinterpret_cast<const V*>(chain_w) + lane + ((wave >> 1) * 8 + (wave & 1) * 4) * 64;
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++) aw[c4 * 4 + kk] = cwp[((int64_t)(gi * 4 + c4) * G3 * 8 + kk) * 64];
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int pos = pos0 + 8 * i, col = col0;
      V v = *reinterpret_cast<const V*>(s_st + pos * kStRowB + col * 16);
      if (has_res) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          h2e p2 = {(_Float16)((float)v[e] + (float)r8[i][e]), (_Float16)((float)v[e + 1] + (float)r8[i][e + 1])};
          p2 = __builtin_elementwise_max(p2, h2e{(_Float16)0.f, (_Float16)0.f});
          v[e] = p2[0];
          v[e + 1] = p2[1];
        }
        *reinterpret_cast<V*>(s_st + pos * kStRowB + col * 16) = v;   // finished rows back to LDS
      }
      if (pos < nvalid) *reinterpret_cast<V*>(reinterpret_cast<char*>(out) + (offg + i * (8 * O * 2))) = v;
    }
    __syncthreads();   // the finished 256-map rows of the tile are in LDS
    // ---- this group's K-slice (channels o0 .. o0 + 255) of the chained GEMM
    if constexpr (C16) {
      V w2[4];
#pragma unroll
      for (int st = 0; st < NG3 * 8; st++) {       // (map group n, chunk c4, k-step): st = n * 8 + c4 * 2 + ks
        constexpr int kLast = NG3 * 8 - 1;
        const int nx = st + 1;
        if (st < kLast) load_w16(chain_w, gi * 4 + ((nx >> 1) & 3), G3, wave + 4 * (nx >> 3), nx & 1, (st & 1) ? aw : w2);
        mma16(s_st + pix16 * kStRowB + ((st >> 1) & 3) * 128 + bofs, 16 * kStRowB, st & 1, (st & 1) ? w2 : aw, cacc[st >> 3]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // wave = 32 maps x 64 positions; K order (chunk, k-step) as the stand-alone OG = 2 launch
#pragma unroll
      for (int c4 = 0; c4 < 4; c4++)
#pragma unroll
        for (int kk = 0; kk < 4; kk++)
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const V bf = *reinterpret_cast<const V*>(s_st + (32 * j + (lane & 31)) * kStRowB + (c4 * 64 + kk * 16 + (lane >> 5) * 8) * 2);
            c2[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aw[c4 * 4 + kk], bf, c2[j], 0, 0, 0);
          }
    }
  }
  __syncthreads();     // every wave is done with the input tile and the staged rows
  // ---- chained result: bias + ReLU, rows staged (O3 * 2 + 16 bytes), whole rows stored 16 B per lane
  constexpr int rowb = O3 * 2 + 16;
  if constexpr (C16) {
#pragma unroll
    for (int n = 0; n < NG3; n++)
#pragma unroll
      for (int a = 0; a < 4; a++) {
        const int och = (wave + 4 * n) * 64 + 16 * a + 4 * kg16;
        const h4e bq = *reinterpret_cast<const h4e*>(chain_b + och);
#pragma unroll
        for (int b = 0; b < 4; b++) {
          h2e lo = {(_Float16)(cacc[n][a][b][0] + (float)bq[0]), (_Float16)(cacc[n][a][b][1] + (float)bq[1])};
          h2e hi = {(_Float16)(cacc[n][a][b][2] + (float)bq[2]), (_Float16)(cacc[n][a][b][3] + (float)bq[3])};
          lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
          hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
          *reinterpret_cast<h4e*>(smem + (16 * b + pix16) * rowb + och * 2) = h4e{lo[0], lo[1], hi[0], hi[1]};
        }
      }
  } else {
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rq = 0; rq < 4; rq++) {
        const int och = wave * 32 + 8 * rq + 4 * (lane >> 5);
        const h4e bq = *reinterpret_cast<const h4e*>(chain_b + och);
        h2e lo = {(_Float16)(c2[j][rq * 4] + (float)bq[0]), (_Float16)(c2[j][rq * 4 + 1] + (float)bq[1])};
        h2e hi = {(_Float16)(c2[j][rq * 4 + 2] + (float)bq[2]), (_Float16)(c2[j][rq * 4 + 3] + (float)bq[3])};
        lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
        hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
        *reinterpret_cast<h4e*>(smem + (32 * j + (lane & 31)) * rowb + och * 2) = h4e{lo[0], lo[1], hi[0], hi[1]};
      }
  }
  __syncthreads();
  constexpr int vpr = O3 / 8;
#pragma unroll
  for (int i = 0; i < kPos * vpr / 256; i++) {
    const int idx = tid + 256 * i, pos = idx / vpr, col = idx % vpr;
    if (g0 + pos < Ntot)
      *reinterpret_cast<V*>(chain_out + (g0 + pos) * O3 + col * 8) = *reinterpret_cast<const V*>(smem + pos * rowb + col * 16);
  }
}

// ------------------------------------------------------------------ 3x3 prediction convs with <= 16 maps, persistent
// odm_reg_head (256 -> 5) and odm_cls_head (256 -> 15), models/head.py:214-222, pyramid-packed.  Their filters are
// zero-padded to 64 rows, and k_conv_f16<9, 1> multiplies all 64: three quarters of its MFMAs are zero rows, and each of
// its four waves pulls the same 8 KB of filter fragments from L2 for every (chunk, tap).  Here only the first 16-row tile
// of the 16x16x32 form runs (the a = 0 MFMAs of k_conv_f16, same B lane map, same K order chunk / tap / k-step, same
// epilogue: every real output has the parent's bits), and the 16-row filter (2 KB per stage, 72 KB at 256 inputs) is
// read out of the SAME packed buffer into LDS once per workgroup.  The workgroups are persistent: each walks a
// contiguous run of 8 x 16 tiles (the halo columns two tiles of a run share are re-read by the same CU; runs of
// workgroups with consecutive ids sit on different XCDs, so the halo rows between runs come through different L2s:
// k_conv_f16's xcd_remap is not applied) and finds the level of every tile anew.  Three buffers hold 64-channel patch
// chunks: while one is computed, the next one has been requested a stage earlier and the one after it -- chunks of the
// next tile included -- is requested now, so two chunks are in flight (with two buffers and one chunk in flight the
// waves waited at every stage's barrier: 43.9 us per launch against 40.2, docs/HISTORY.md "Round 8").
// A wave owns two patch rows (2 x 16 positions): three ds_read_b128 per two MFMAs.
constexpr int kNarrowPatch = ConvCfg<9, 1>::kPatchBytes;                  // 10 x 18 pixels x 144 B, in 1 KB DMA pieces
constexpr int kNarrowJ = ConvCfg<9, 1>::kJ;
constexpr int kNarrowDma = ConvCfg<9, 1>::kDma;
constexpr int kNarrowOutBytes = 128 * 32;                                 // staged tile: 128 positions x 16 maps
constexpr int kNarrowFixedLds = 3 * kNarrowPatch + 2 * kNarrowOutBytes + 64;  // three patch chunks: two in flight
constexpr int kNarrowMaxC = 256;                                          // 18 KB of filter per 64 inputs: 161 856 B of 160 KiB
inline int narrow_lds_bytes(int C) { return kNarrowFixedLds + (C / 64) * 9 * 2048; }

__global__ __launch_bounds__(256, 1) void k_conv3x3_narrow_f16(const _Float16* __restrict__ x,
                                                               const _Float16* __restrict__ wfrag,
                                                               const _Float16* __restrict__ bias,
                                                               _Float16* __restrict__ out, int C, int O_used, int relu,
                                                               unsigned x_bytes, LevelTab lt, int tiles) {
  using T = _Float16;
  using V = f16x8;
  using h2e = __attribute__((ext_vector_type(2))) _Float16;
  using h4e = __attribute__((ext_vector_type(4))) _Float16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int CC = C / 64, nstage = 9 * CC;
  char* s_w = smem + 3 * kNarrowPatch;                 // [stage][k-step][lane] x 16 B
  char* s_out = s_w + nstage * 2048;                   // two staged tiles (by tile parity)
  T* s_bias = reinterpret_cast<T*>(s_out + 2 * kNarrowOutBytes);
  // this workgroup's run of tiles
  const int t_begin = (int)((int64_t)blockIdx.x * tiles / gridDim.x);
  const int t_end = (int)((int64_t)(blockIdx.x + 1) * tiles / gridDim.x);
  if (t_begin >= t_end) return;
  const unsigned row_bytes = (unsigned)C * 2;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(x), 0, (int)x_bytes, 0x00020000);

  struct Tile { int H, W, ty0, tx0; int64_t base; };   // base: packed pixel index of (image, 0, 0)
  auto decode = [&](int tile) {
    int t0 = 0, p0 = 0, H = lt.H[0], W = lt.W[0];
#pragma unroll
    for (int i = 1; i < kMaxLevels; i++)
      if (i < lt.n && tile >= lt.tile0[i]) {
        t0 = lt.tile0[i]; p0 = lt.pix0[i]; H = lt.H[i]; W = lt.W[i];
      }
    const int txn = (W + 15) / 16, tyn = (H + 7) / 8, loc = tile - t0;
    const int bimg = loc / (txn * tyn), trem = loc % (txn * tyn);
    return Tile{H, W, (trem / txn) * 8, (trem % txn) * 16, (int64_t)p0 + (int64_t)bimg * H * W};
  };
  // patch chunk -> LDS by LDS-DMA: slot layout and zero fill of k_conv_f16 (pixel * 9 + 16-byte piece, pad piece and
  // pixels outside the image read out of range), one buffer descriptor over the whole packed input
  unsigned pvoff[kNarrowJ];
  auto bind = [&](const Tile& tl) {
#pragma unroll
    for (int j = 0; j < kNarrowJ; j++) {
      const int v = (wave_u + 4 * j) * 64 + lane, p = v / 9, q = v % 9;
      const int yy = tl.ty0 - 1 + p / kCPW, xx = tl.tx0 - 1 + p % kCPW;
      const bool in = q < 8 && p < ConvCfg<9, 1>::kPix && yy >= 0 && yy < tl.H && xx >= 0 && xx < tl.W;
      pvoff[j] = in ? (unsigned)((tl.base + (int64_t)yy * tl.W + xx) * row_bytes + q * 16) : 0x80000000u;
    }
  };
  auto piece_issue = [&](int buf, int cc, int j) {      // piece j of this wave (7 cover the 26 of a chunk)
    const int i = wave_u + 4 * j;
    if (i < kNarrowDma)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(smem + buf * kNarrowPatch + i * 1024),
                                               16, (int)pvoff[j], cc * 128, 0, 0);
  };
  auto patch_issue = [&](int buf, int cc) {
#pragma unroll
    for (int j = 0; j < kNarrowJ; j++) piece_issue(buf, cc, j);
  };

  // issue cursor: the chunk that is requested next, two ahead of the one being computed
  int itile = t_begin, icc = 0;
  bool ivalid = true;
  auto advance = [&]() {
    if (++icc == CC) {
      icc = 0;
      if (++itile < t_end) bind(decode(itile)); else ivalid = false;
    }
  };
  bind(decode(t_begin));
  patch_issue(0, 0);
  advance();
  if (ivalid) {
    patch_issue(1, icc);
    advance();
  }
  // rows 0..15 of the packed filter: (stage s, k-step ks, lane l) is the fragment load_w reads for tile a = 0
  for (int idx = tid; idx < nstage * 128; idx += 256) {
    const int s = idx >> 7, ks = (idx >> 6) & 1, l = idx & 63;
    *reinterpret_cast<V*>(s_w + idx * 16) =
        reinterpret_cast<const V*>(wfrag)[(int64_t)s * 512 + ks * 64 + ((l >> 4) & 1) * 128 + (l >> 5) * 32 + (l & 15)];
  }
  if (tid < 16) s_bias[tid] = (bias && tid < O_used) ? bias[tid] : (T)0.f;

  // lane maps of the 16x16x32 form (k_conv_f16): position pix16 of patch row 2 * wave + b, k-group kg16
  const int kg16 = lane >> 4, i16 = lane & 15;
  const int pix16 = (i16 >= 4 && i16 < 12) ? (((i16 - 4) >> 1) * 4 + (i16 & 1))
                                           : (((i16 & 3) >> 1) * 4 + 2 + (i16 & 1) + (i16 >= 12 ? 8 : 0));
  const int fbase16 = (2 * wave * kCPW + pix16) * kRowBytes + (kg16 & 1) * 64 + (kg16 >> 1) * 16;
  constexpr int kTile16 = kCPW * kRowBytes;
  const bool relu_u = __builtin_amdgcn_readfirstlane(relu) != 0;
  f32x4 acc[2];
#pragma unroll
  for (int b = 0; b < 2; b++)
#pragma unroll
    for (int r = 0; r < 4; r++) acc[b][r] = 0.f;
  __syncthreads();      // first chunk, filter and bias in LDS

  // end of a stage: this wave's pieces of the NEXT chunk have landed (vmcnt counts loads in order: only the pieces
  // issued during this stage, `newest` of them, may still be in flight), its LDS writes are done, then the barrier.
  // Written as one asm statement: in front of a barrier of its own the compiler waits for vmcnt(0), which would take
  // the second chunk in flight away again.
  auto stage_sync = [&](bool issued) {
    __builtin_amdgcn_sched_barrier(0);
    if (!issued) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else if (wave_u + 4 * (kNarrowJ - 1) < kNarrowDma) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };
  static_assert(kNarrowJ == 7 && kNarrowDma == 26, "stage_sync counts 7 pieces on waves 0-1 and 6 on waves 2-3");
  int rb = 0;
  for (int tile = t_begin; tile < t_end; tile++) {
    const Tile cur = decode(tile);
    bool issued = false;
    for (int cc = 0; cc < CC; cc++) {
      // the chunk two stages ahead (of this tile or of a later one) goes into the buffer every wave left at the last
      // barrier: one DMA piece per tap, between the MFMAs
      const bool more = ivalid;
      issued = more;
      const int ncc = icc, wb = rb == 0 ? 2 : rb - 1, buf = rb;
      const char* P = smem + buf * kNarrowPatch + fbase16;
      const char* Wc = s_w + cc * (9 * 2048) + lane * 16;
      // fragments two taps ahead in registers (one wave per SIMD: nothing else covers the LDS latency)
      V fa[3][2], fp[3][2][2];
      auto load_tap = [&](int t, V (&a)[2], V (&p)[2][2]) {
        const int toff = ((t / 3) * kCPW + (t % 3)) * kRowBytes;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
          a[ks] = *reinterpret_cast<const V*>(Wc + (t * 2 + ks) * 1024);
          p[ks][0] = *reinterpret_cast<const V*>(P + toff + ks * 32);
          p[ks][1] = *reinterpret_cast<const V*>(P + kTile16 + toff + ks * 32);
        }
      };
      load_tap(0, fa[0], fp[0]);
      load_tap(1, fa[1], fp[1]);
#pragma unroll
      for (int t = 0; t < 9; t++) {
        if (t + 2 < 9) load_tap(t + 2, fa[(t + 2) % 3], fp[(t + 2) % 3]);
        if (t < kNarrowJ && more) piece_issue(wb, ncc, t);
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
          acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[t % 3][ks], fp[t % 3][ks][0], acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[t % 3][ks], fp[t % 3][ks][1], acc[1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (more) advance();                // (rebinds the patch offsets when the cursor enters a new tile)
      rb = rb == 2 ? 0 : rb + 1;
      if (cc + 1 < CC) stage_sync(more);  // the next chunk has landed; the buffer just read is free
    }
    // ---- epilogue of k_conv_f16: f32 sum + f16 bias, one f16 rounding, ReLU on the rounded halves; maps >= O_used are +0
    char* so = s_out + ((tile - t_begin) & 1) * kNarrowOutBytes;
    {
      const int och = 4 * kg16;                      // D: row (out channel) = 4 (lane >> 4) + register, column = pixel
      const h4e bq = *reinterpret_cast<const h4e*>(s_bias + och);
#pragma unroll
      for (int b = 0; b < 2; b++) {
        h2e lo = {(_Float16)(acc[b][0] + (float)bq[0]), (_Float16)(acc[b][1] + (float)bq[1])};
        h2e hi = {(_Float16)(acc[b][2] + (float)bq[2]), (_Float16)(acc[b][3] + (float)bq[3])};
        if (relu_u) {
          lo = __builtin_elementwise_max(lo, h2e{(_Float16)0.f, (_Float16)0.f});
          hi = __builtin_elementwise_max(hi, h2e{(_Float16)0.f, (_Float16)0.f});
        }
        h4e v4 = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
        for (int e = 0; e < 4; e++)
          if (och + e >= O_used) v4[e] = (_Float16)0.f;
        *reinterpret_cast<h4e*>(so + (16 * (2 * wave + b) + pix16) * 32 + och * 2) = v4;
#pragma unroll
        for (int r = 0; r < 4; r++) acc[b][r] = 0.f;
      }
    }
    stage_sync(issued);   // tile staged; the next tile's first chunk has landed and the buffer just read is free
    // whole 128-byte rows: two vectors of maps, six of zeros (the 64-column buffer's padding, written as the parent does)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int idx = tid + 256 * i, pos = idx >> 3, col = idx & 7;
      const int y = cur.ty0 + (pos >> 4), xq = cur.tx0 + (pos & 15);
      V v;
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = (_Float16)0.f;
      if (col < 2) v = *reinterpret_cast<const V*>(so + pos * 32 + col * 16);
      if (y < cur.H && xq < cur.W) *reinterpret_cast<V*>(out + (cur.base + (int64_t)y * cur.W + xq) * 64 + col * 8) = v;
    }
  }
}

}  // namespace
}  // namespace s2a

using namespace s2a;

namespace s2a {
namespace {
template <int TAPS, int OG, int PH = 1, int SD = 1, bool TAIL = false, int HT = 0>
int launch_conv(const _Float16* x, const _Float16* wfrag, const _Float16* bias, const _Float16* residual,
                _Float16* out, int64_t B, int C, int H, int W, int Ho, int Wo, int cstride, int O, int relu,
                hipStream_t st, const LevelTab* levels = nullptr, int64_t level_tiles = 0, int res_up = 0,
                ConvExtra ex = ConvExtra{nullptr, nullptr, nullptr, nullptr, 1}) {
  using Cfg = ConvCfg<TAPS, OG, PH, SD, TAIL, HT>;
  const int64_t Ntot = B * (int64_t)Ho * Wo;
  int64_t tiles = TAPS == 9 ? B * ((Wo + 15) / 16) * ((Ho + Cfg::kTH - 1) / Cfg::kTH) : (Ntot + Cfg::kPos - 1) / Cfg::kPos;
  LevelTab lt = {};
  if (levels) { lt = *levels; tiles = level_tiles; }
  dim3 grid((unsigned)tiles, (unsigned)((O + 64 * OG - 1) / (64 * OG)));
  auto kern = k_conv_f16<TAPS, OG, PH, SD, TAIL, HT>;
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::kLds + Cfg::kBiasBytes));
  kern<<<grid, 256 * PH, Cfg::kLds + Cfg::kBiasBytes, st>>>(x, wfrag, bias, residual, out, Ntot, C, H, W, Ho, Wo, cstride, O, relu,
                                     (unsigned)((uint64_t)B * H * W * C * 2), lt, res_up, ex);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

// the template arguments of k_conv_f16 as a value: what the conv_form_*() functions decide and ConvCall::run(form) launches
struct ConvForm {
  int taps, og, ph, sd, tail, ht;
  bool operator==(const ConvForm& o) const {
    return taps == o.taps && og == o.og && ph == o.ph && sd == o.sd && tail == o.tail && ht == o.ht;
  }
};

// the arguments of one launch_conv call: an entry point fills them once and hands the form it decided to run(form)
struct ConvCall {
  const _Float16 *x, *wfrag, *bias, *residual;
  _Float16* out;
  int64_t B;
  int C, H, W, Ho, Wo, cstride, O, relu;
  hipStream_t st;
  const LevelTab* levels = nullptr;
  int64_t level_tiles = 0;
  int res_up = 0;
  ConvExtra ex = ConvExtra{nullptr, nullptr, nullptr, nullptr, 1};
  template <int TAPS, int OG, int PH = 1, int SD = 1, bool TAIL = false, int HT = 0>
  int run() const {
    return launch_conv<TAPS, OG, PH, SD, TAIL, HT>(x, wfrag, bias, residual, out, B, C, H, W, Ho, Wo, cstride, O, relu, st, levels,
                                                   level_tiles, res_up, ex);
  }
  // THE list of the k_conv_f16 instantiations this file builds; a form outside it is refused in front of any launch
  int run(const ConvForm& f) const {
#define S2A_CONV_FORM(TAPS, OG, PH, SD, TAIL, HT) \
  if (f == ConvForm{TAPS, OG, PH, SD, TAIL, HT}) return run<TAPS, OG, PH, SD, TAIL, HT>()
    S2A_CONV_FORM(9, 4, 1, 2, 0, 0);   // 3x3 stride 2
    S2A_CONV_FORM(9, 2, 1, 2, 0, 0);
    S2A_CONV_FORM(9, 2, 2, 1, 0, 0);   // 3x3 on 16 x 16 tiles, the filter through LDS
    S2A_CONV_FORM(9, 1, 2, 1, 0, 0);
    S2A_CONV_FORM(9, 4, 2, 1, 0, 0);
    S2A_CONV_FORM(9, 4, 1, 1, 0, 1);   // 3x3 on 4 x 16 tiles
    S2A_CONV_FORM(9, 2, 1, 1, 0, 1);
    S2A_CONV_FORM(9, 4, 1, 1, 0, 0);   // 3x3 on 8 x 16 tiles
    S2A_CONV_FORM(9, 2, 1, 1, 0, 0);
    S2A_CONV_FORM(9, 1, 1, 1, 0, 0);
    S2A_CONV_FORM(1, 4, 1, 2, 0, 0);   // 1x1 on 64 positions
    S2A_CONV_FORM(1, 4, 1, 1, 0, 0);   // 1x1 on 128 positions
    S2A_CONV_FORM(1, 2, 1, 1, 0, 0);
    S2A_CONV_FORM(1, 1, 1, 1, 0, 0);
    S2A_CONV_FORM(9, 1, 2, 1, 1, 0);   // 3x3 + the bottleneck's 1x1 tail, 16 x 16 and 8 x 16 tiles
    S2A_CONV_FORM(9, 1, 1, 1, 1, 0);
#undef S2A_CONV_FORM
    s2a::set_error("conv: no kernel of form <%d, %d, %d, %d, %d, %d>", f.taps, f.og, f.ph, f.sd, f.tail, f.ht);
    return S2A_EINVAL;
  }
};

// ---- which form a call launches: host arithmetic and getenv only.  The tile-shape switches are A/B switches for
// measurements and tests, which flip them between calls of one process: the environment is read on every call.
// S2A_CONV_PH, S2A_CONV_PH_NARROW = 1|2: any set value other than 2 is 1
inline int env_ph(const char* name, int ph) {
  const char* f = getenv(name);
  return f ? (atoi(f) == 2 ? 2 : 1) : ph;
}
// S2A_CONV3_HALF, S2A_CONV1_HALF = 0|1
inline bool env_flag(const char* name, bool on) {
  const char* f = getenv(name);
  return f ? atoi(f) != 0 : on;
}
inline int conv_og(int64_t out_channels) { return out_channels % 256 == 0 ? 4 : (out_channels % 128 == 0 ? 2 : 1); }

// s2a_conv_nhwc_f16 (and its query s2a_conv_nhwc_f16_form), for sizes that conv_nhwc_check_sizes lets through
ConvForm conv_form_nhwc(int64_t batch, int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                        int stride) {
  const int64_t Ho = (height - 1) / stride + 1, Wo = (width - 1) / stride + 1;   // k=1,p=0 / k=3,p=1 (s = 1, 2)
  const int og = conv_og(out_channels);
  const int64_t groups = (out_channels + 64 * og - 1) / (64 * og);
  if (ksize == 3 && stride == 2) return {9, og == 4 ? 4 : 2, 1, 2, 0, 0};
  if (ksize == 3 && og < 4 && channels % 64 == 0) {
    // narrow 3x3 layers (the 64- and 128-map conv2 of the trunk's first stages): the four waves of an 8 x 16 tile
    // re-load the same filter fragments (4x / 2x the bytes into the CU); 16 x 16 tiles with the filter of each tap
    // staged once per workgroup through LDS when there are enough tiles to fill the chip.  S2A_CONV_PH_NARROW=1|2
    const int64_t tiles16 = batch * ((Wo + 15) / 16) * ((Ho + 15) / 16) * groups;
    if (env_ph("S2A_CONV_PH_NARROW", tiles16 >= 256 ? 2 : 1) == 2) return {9, og, 2, 1, 0, 0};
  }
  if (ksize == 3 && og == 4 && channels % 64 == 0) {
    // large maps (FPN's 3x3 on P3: 128^2 at batch 8): 16 x 16 tiles with the filter through LDS, as the pyramid-packed
    // towers -- when they still fill the chip twice.  S2A_CONV_PH=1|2
    const int64_t tiles16 = batch * ((Wo + 15) / 16) * ((Ho + 15) / 16) * groups;
    if (env_ph("S2A_CONV_PH", tiles16 >= 512 ? 2 : 1) == 2) return {9, 4, 2, 1, 0, 0};
  }
  if (ksize == 3 && og >= 2) {
    // small maps (32^2 at batch 8): fewer 8 x 16 workgroups than CUs -> 4 x 16 tiles (512 -> 512 on 32^2: 54 -> 44 us,
    // 256 -> 256 on 32^2: 28 -> 19 us; once every CU has a workgroup the smaller tile loses: 256 -> 256 on 64^2
    // 39.5 -> 43 us).  S2A_CONV3_HALF=0|1
    const int64_t wgs128 = batch * ((Wo + 15) / 16) * ((Ho + 7) / 8) * groups;
    if (env_flag("S2A_CONV3_HALF", wgs128 < 256)) return {9, og, 1, 1, 0, 1};
  }
  if (ksize == 3) return {9, og, 1, 1, 0, 0};
  if (og == 4) {
    // small maps (64^2 / 32^2 at batch 8): 128-position tiles give at most one workgroup per CU, and one workgroup's
    // chunk pipeline is latency-bound (32 MFMAs per wave between two memory round trips) -- 64-position tiles fill
    // the chip (2048 -> 512 and 2048 -> 256 on 32^2: 35 -> 26 us, 34 -> 23 us; no gain once every CU has a workgroup).  (ConvCfg<1, 4, 1, 2>: SD = 2 selects the 64-position tile; the spatial
    // stride of a 1x1 is the cstride argument.)  S2A_CONV1_HALF=0|1
    const int64_t wgs128 = (batch * Ho * Wo + 127) / 128 * groups;
    // measured: a win only while the 128-position grid leaves CUs empty
    if (env_flag("S2A_CONV1_HALF", wgs128 < 256)) return {1, 4, 1, 2, 0, 0};
  }
  return {1, og, 1, 1, 0, 0};
}

// s2a_conv1x1_add_up2_f16: the 128-position 1x1 of the width
ConvForm conv_form_up2(int64_t out_channels) { return {1, conv_og(out_channels), 1, 1, 0, 0}; }

// the pyramid-packed 3x3 launches (conv3x3_pyramid_impl); has_head: a 1x1 prediction head is fused on the tile
ConvForm conv_form_pyramid(int64_t channels, int64_t out_channels, bool has_head) {
  int og = conv_og(out_channels);
  // A/B switch for measurements; not for the fused 1x1 head, which needs the whole channel range in one workgroup (OG = 4)
  const char* og_env = getenv("S2A_CONV_OG");
  if (og_env && !has_head) og = std::min(og, std::max(1, atoi(og_env)));
  if (og == 3) og = 1;   // (there is no three-group kernel: capped at 3, a 256-map layer runs one group per workgroup)
  // Full-width towers: 16 x 16 tiles on 512-thread workgroups with the filter staged once per workgroup through
  // LDS (ConvCfg::kWLds) -- 4-7 % faster than two 8 x 16 workgroups per CU, bit-identical.  S2A_CONV_PH=1|2: A/B switch.
  // Only the OG = 4 form has 16-row tiles: the level table must be built for the tile height that is launched.
  const int ph = (og == 4 && channels % 64 == 0) ? env_ph("S2A_CONV_PH", 2) : 1;
  return {9, og, ph, 1, 0, 0};
}

// s2a_conv3x3_tail1x1_f16: 16 x 16 tiles when they fill the chip, as the narrow 3x3 layers.  S2A_CONV_PH_NARROW=1|2
ConvForm conv_form_tail(int64_t batch, int64_t height, int64_t width) {
  const int64_t tiles16 = batch * ((width + 15) / 16) * ((height + 15) / 16);
  return {9, 1, env_ph("S2A_CONV_PH_NARROW", tiles16 >= 256 ? 2 : 1), 1, 1, 0};
}

// the checks of s2a_conv_nhwc_f16 that read sizes only, shared with its query
int conv_nhwc_check_sizes(int64_t batch, int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                          int stride, bool has_residual) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0 && height > 0 && width > 0, "conv: bad shape");
  S2A_CHECK_ARG(ksize == 3 || ksize == 1, "conv: kernel size must be 1 or 3");
  S2A_CHECK_ARG(stride == 1 || stride == 2, "conv: stride must be 1 or 2");
  S2A_CHECK_ARG(!(ksize == 3 && stride == 2) || out_channels % 128 == 0, "conv: 3x3 stride 2 needs out_channels % 128 == 0");
  S2A_CHECK_ARG((channels % 64 == 0 || channels == 32) && out_channels % 64 == 0,
                "conv: channels must be 32 or a multiple of 64, out_channels a multiple of 64");
  const uint64_t x_bytes = (uint64_t)batch * height * width * channels * 2;
  S2A_CHECK_ARG(x_bytes < (1ull << 31) && (ksize == 1 || (height < 32000 && width < 32000)),
                "conv: input too large for 32-bit offsets");
  S2A_CHECK_ARG(!has_residual || (uint64_t)batch * ((height - 1) / stride + 1) * ((width - 1) / stride + 1) * out_channels * 2 < (1ull << 31),
                "conv: output too large for the fused residual (32-bit offsets)");
  return S2A_OK;
}
}  // namespace
}  // namespace s2a

// the query: the entry point's own size checks and the conv_form_nhwc call it dispatches on.  (Only a call with a residual
// bounds the output's size; the query takes none, as a call without one.)
extern "C" int s2a_conv_nhwc_f16_form(int64_t batch, int64_t channels, int64_t height, int64_t width, int64_t out_channels,
                                      int ksize, int stride, int32_t form[6]) {
  if (int rc = conv_nhwc_check_sizes(batch, channels, height, width, out_channels, ksize, stride, false)) return rc;
  S2A_CHECK_ARG(form, "conv_form: NULL form");
  const ConvForm f = conv_form_nhwc(batch, channels, height, width, out_channels, ksize, stride);
  form[0] = f.taps, form[1] = f.og, form[2] = f.ph, form[3] = f.sd, form[4] = f.tail, form[5] = f.ht;
  return S2A_OK;
}

extern "C" int s2a_conv_nhwc_f16(const void* x, const void* weight_frag, const void* bias, const void* residual,
                                 void* out, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                 int64_t out_channels, int ksize, int stride, int relu, s2a_stream_t stream) {
  if (int rc = conv_nhwc_check_sizes(batch, channels, height, width, out_channels, ksize, stride, residual != nullptr)) return rc;
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && out, "conv: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)bias % 8) == 0 && ((uintptr_t)residual % 16) == 0, "conv: tensors must be 16-byte aligned");
  const int Ho = (int)((height - 1) / stride + 1), Wo = (int)((width - 1) / stride + 1);   // k=1,p=0 / k=3,p=1 (s = 1, 2)
  const ConvCall c{(const _Float16*)x, (const _Float16*)weight_frag, (const _Float16*)bias, (const _Float16*)residual,
                   (_Float16*)out, batch, (int)channels, (int)height, (int)width, Ho, Wo, stride, (int)out_channels, relu,
                   as_stream(stream)};
  return c.run(conv_form_nhwc(batch, channels, height, width, out_channels, ksize, stride));
}

extern "C" int s2a_conv3x3_tail1x1_f16(const void* x, const void* weight_frag, const void* bias,
                                       const void* tail_weight_frag, const void* tail_bias, const void* residual,
                                       void* out, const void* chain_weight_frag, const void* chain_bias, void* chain_out,
                                       int64_t chain_channels, int64_t batch, int64_t channels, int64_t mid_channels,
                                       int64_t out_channels, int64_t height, int64_t width, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && height > 0 && width > 0, "conv3x3_tail1x1: bad shape");
  S2A_CHECK_ARG(channels == 64 && mid_channels == 64 && out_channels == 256,
                "conv3x3_tail1x1: built for the 64 -> 64 -> 256 bottleneck tail");
  S2A_CHECK_ARG((uint64_t)batch * height * width * out_channels * 2 < (1ull << 31) && height < 32000 && width < 32000,
                "conv3x3_tail1x1: tensor too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && bias && tail_weight_frag && tail_bias && out, "conv3x3_tail1x1: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)tail_weight_frag % 16) == 0 && ((uintptr_t)bias % 8) == 0 && ((uintptr_t)tail_bias % 8) == 0 &&
                ((uintptr_t)residual % 16) == 0, "conv3x3_tail1x1: tensors must be 16-byte aligned");
  ConvExtra ex{};
  ex.store_main = 0;
  ex.tail_w = (const _Float16*)tail_weight_frag;
  ex.tail_b = (const _Float16*)tail_bias;
  ex.tail_res = (const _Float16*)residual;
  ex.tail_out = (_Float16*)out;
  if (chain_weight_frag || chain_bias || chain_out) {
    S2A_CHECK_ARG(chain_weight_frag && chain_bias && chain_out, "conv3x3_tail1x1: chain filter, bias and output go together");
    S2A_CHECK_ARG(chain_channels == 64 || chain_channels == 128, "conv3x3_tail1x1: the chained 1x1 has 64 or 128 maps");
    S2A_CHECK_ARG(((uintptr_t)chain_weight_frag % 16) == 0 && ((uintptr_t)chain_bias % 8) == 0 && ((uintptr_t)chain_out % 16) == 0,
                  "conv3x3_tail1x1: chain tensors must be 16-byte aligned");
    ex.chain_w = (const _Float16*)chain_weight_frag;
    ex.chain_b = (const _Float16*)chain_bias;
    ex.chain_out = (_Float16*)chain_out;
    ex.chain_O = (int)chain_channels;
  }
  const ConvCall c{(const _Float16*)x, (const _Float16*)weight_frag, (const _Float16*)bias, nullptr, (_Float16*)out, batch, 64,
                   (int)height, (int)width, (int)height, (int)width, 1, 64, 1, as_stream(stream), nullptr, 0, 0, ex};
  return c.run(conv_form_tail(batch, height, width));
}

namespace s2a {
namespace {
template <int CC, int O3>
int launch_conv1x1_chain(const _Float16* x, const _Float16* wfrag, const _Float16* bias, const _Float16* residual, _Float16* out,
                         const _Float16* cw, const _Float16* cb, _Float16* cout, int64_t P, hipStream_t st) {
  constexpr int K = 64 * CC;
  const int loop = CC * 64 * kRowBytes + 64 * 528 + 512;      // input tile + staged 256-map rows + bias
  const int tail = 64 * (O3 * 2 + 16);                              // staged rows of the chained result (over the tile)
  const int lds = loop > tail ? loop : tail;
  auto kern = k_conv1x1_chain_f16<CC, O3>;
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  kern<<<dim3((unsigned)((P + 63) / 64)), 256, lds, st>>>(x, wfrag, bias, residual, out, cw, cb, cout, P,
                                                          (unsigned)((uint64_t)P * K * 2));
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
}  // namespace
}  // namespace s2a

extern "C" int s2a_conv1x1_chain_f16(const void* x, const void* weight_frag, const void* bias, const void* residual,
                                     void* out, const void* chain_weight_frag, const void* chain_bias, void* chain_out,
                                     int64_t chain_channels, int64_t batch, int64_t channels, int64_t out_channels,
                                     int64_t height, int64_t width, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && height > 0 && width > 0, "conv1x1_chain: bad shape");
  S2A_CHECK_ARG((channels == 128 && out_channels == 512 && (chain_channels == 128 || chain_channels == 256)) ||
                (channels == 256 && out_channels == 1024 && chain_channels == 256),
                "conv1x1_chain: built for (K, O, O3) = (128, 512, 128), (128, 512, 256), (256, 1024, 256)");
  S2A_CHECK_ARG((uint64_t)batch * height * width * out_channels * 2 < (1ull << 31),
                "conv1x1_chain: tensor too large for 32-bit offsets");
  S2A_CHECK_ARG((chain_weight_frag && chain_bias && chain_out) || (!chain_weight_frag && !chain_bias && !chain_out),
                "conv1x1_chain: chain filter, bias and output go together");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && bias && out && chain_weight_frag, "conv1x1_chain: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)bias % 8) == 0 && ((uintptr_t)residual % 16) == 0 && ((uintptr_t)chain_weight_frag % 16) == 0 &&
                ((uintptr_t)chain_bias % 8) == 0 && ((uintptr_t)chain_out % 16) == 0,
                "conv1x1_chain: tensors must be 16-byte aligned");
  const int64_t P = batch * height * width;
  const _Float16 *X = (const _Float16*)x, *Wf = (const _Float16*)weight_frag, *Bi = (const _Float16*)bias,
                 *R = (const _Float16*)residual, *Cw = (const _Float16*)chain_weight_frag, *Cb = (const _Float16*)chain_bias;
  hipStream_t st = as_stream(stream);
  if (channels == 256) return launch_conv1x1_chain<4, 256>(X, Wf, Bi, R, (_Float16*)out, Cw, Cb, (_Float16*)chain_out, P, st);
  if (chain_channels == 128) return launch_conv1x1_chain<2, 128>(X, Wf, Bi, R, (_Float16*)out, Cw, Cb, (_Float16*)chain_out, P, st);
  return launch_conv1x1_chain<2, 256>(X, Wf, Bi, R, (_Float16*)out, Cw, Cb, (_Float16*)chain_out, P, st);
}

extern "C" int s2a_conv1x1_add_up2_f16(const void* x, const void* weight_frag, const void* bias, const void* coarse,
                                       void* out, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                       int64_t out_channels, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0 && height > 0 && width > 0, "conv_add_up2: bad shape");
  S2A_CHECK_ARG(height % 2 == 0 && width % 2 == 0, "conv_add_up2: the map must be exactly twice the coarse map");
  S2A_CHECK_ARG(channels % 64 == 0 && out_channels % 64 == 0, "conv_add_up2: channel counts must be multiples of 64");
  const uint64_t x_bytes = (uint64_t)batch * height * width * channels * 2;
  S2A_CHECK_ARG(x_bytes < (1ull << 31) && (uint64_t)batch * height * width * out_channels * 2 < (1ull << 31),
                "conv_add_up2: tensor too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && coarse && out, "conv_add_up2: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)bias % 2) == 0 && ((uintptr_t)coarse % 16) == 0, "conv_add_up2: tensors must be 16-byte aligned");
  const ConvCall c{(const _Float16*)x, (const _Float16*)weight_frag, (const _Float16*)bias, (const _Float16*)coarse,
                   (_Float16*)out, batch, (int)channels, (int)height, (int)width, (int)height, (int)width, 1, (int)out_channels, 0,
                   as_stream(stream), nullptr, 0, 1};
  return c.run(conv_form_up2(out_channels));
}

extern "C" int s2a_conv_pack_weight_f16(const void* weight, int64_t out_channels, int64_t channels, int ksize,
                                        void* packed, s2a_stream_t stream) {
  S2A_CHECK_ARG(ksize == 3 || ksize == 1, "conv_pack_weight: kernel size must be 1 or 3");
  S2A_CHECK_ARG(out_channels % 64 == 0 && channels % 64 == 0, "conv_pack_weight: channel counts must be multiples of 64");
  S2A_CHECK_ARG(weight && packed, "conv_pack_weight: NULL tensor");
  const int taps = ksize * ksize;
  const int64_t wtot = out_channels * channels * taps;
  k_pack_weight_frag<<<(unsigned)((wtot + 255) / 256), 256, 0, as_stream(stream)>>>(
      (const _Float16*)weight, (int)out_channels, (int)channels, (_Float16*)packed, taps);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

// ------------------------------------------------------------------ pyramid-packed launches
extern "C" int64_t s2a_pyramid_pixels(const s2a_pyramid* pyr, int64_t batch) {
  LevelTab lt; int64_t pix = 0;
  return build_levels(pyr, batch, &lt, &pix) < 0 ? -1 : pix;
}

static int conv3x3_pyramid_impl(const void* x, const void* weight_frag, const void* bias, const void* residual,
                                void* out, ConvExtra ex, int64_t batch, int64_t channels, int64_t out_channels,
                                int relu, const s2a_pyramid* pyr, s2a_stream_t stream);

extern "C" int s2a_conv3x3_pyramid_f16(const void* x, const void* weight_frag, const void* bias, const void* residual,
                                       void* out, int64_t batch, int64_t channels, int64_t out_channels,
                                       int relu, const s2a_pyramid* pyr, s2a_stream_t stream) {
  return conv3x3_pyramid_impl(x, weight_frag, bias, residual, out, ConvExtra{nullptr, nullptr, nullptr, nullptr, 1}, batch,
                              channels, out_channels, relu, pyr, stream);
}

extern "C" int s2a_conv3x3_head_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out,
                                            const void* head_weight_frag, const void* head_bias, void* head_out,
                                            int64_t batch, int64_t channels, int64_t out_channels, int relu,
                                            const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(out_channels == 256, "conv3x3_head_pyramid: the fused 1x1 head needs a 256-channel tower");
  S2A_CHECK_ARG(head_weight_frag && head_bias && head_out, "conv3x3_head_pyramid: NULL head tensor");
  S2A_CHECK_ARG(((uintptr_t)head_weight_frag % 16) == 0 && ((uintptr_t)head_bias % 8) == 0 && ((uintptr_t)head_out % 16) == 0,
                "conv3x3_head_pyramid: misaligned head tensor");
  ConvExtra ex{nullptr, (const _Float16*)head_weight_frag, (const _Float16*)head_bias, (_Float16*)head_out, out != nullptr};
  return conv3x3_pyramid_impl(x, weight_frag, bias, nullptr, out ? out : head_out, ex, batch, channels, out_channels, relu,
                              pyr, stream);
}

extern "C" int s2a_orconv_pool_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out,
                                           void* pooled, int64_t batch, int64_t channels, int64_t out_channels,
                                           const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(pooled != nullptr && ((uintptr_t)pooled % 16) == 0 && out_channels % 64 == 0,
                "orconv_pool_pyramid: pooled must be a 16-byte aligned buffer, out_channels a multiple of 64");
  return conv3x3_pyramid_impl(x, weight_frag, bias, nullptr, out, ConvExtra{(_Float16*)pooled, nullptr, nullptr, nullptr, 1},
                              batch, channels, out_channels, 0, pyr, stream);
}

static int conv3x3_pyramid_impl(const void* x, const void* weight_frag, const void* bias, const void* residual,
                                void* out, ConvExtra ex, int64_t batch, int64_t channels, int64_t out_channels,
                                int relu, const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0 && out_channels > 0, "conv_pyramid: bad shape");
  S2A_CHECK_ARG((channels % 64 == 0 || channels == 32) && out_channels % 64 == 0,
                "conv_pyramid: channels must be 32 or a multiple of 64, out_channels a multiple of 64");
  LevelTab lt; int64_t pix = 0;
  const ConvForm form = conv_form_pyramid(channels, out_channels, ex.head_w != nullptr);
  const int64_t tiles = build_levels(pyr, batch, &lt, &pix, 8 * form.ph);
  S2A_CHECK_ARG(tiles >= 0, "conv_pyramid: bad level table (1..8 levels, positive sizes)");
  S2A_CHECK_ARG((uint64_t)pix * channels * 2 < (1ull << 31), "conv_pyramid: input too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && out, "conv_pyramid: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)bias % 8) == 0 && ((uintptr_t)residual % 16) == 0, "conv_pyramid: tensors must be 16-byte aligned");
  if (lt.n == 1) lt.n = 2, lt.tile0[1] = 0x7fffffff;   // keep the rebind path (n > 1) for a one-level table
  const ConvCall c{(const _Float16*)x, (const _Float16*)weight_frag, (const _Float16*)bias, (const _Float16*)residual,
                   (_Float16*)out, batch, (int)channels, lt.H[0], lt.W[0], lt.H[0], lt.W[0], 1, (int)out_channels, relu,
                   as_stream(stream), &lt, tiles, 0, ex};
  return c.run(form);
}

extern "C" int s2a_conv3x3_narrow_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out,
                                              int64_t batch, int64_t channels, int64_t out_channels_used, int relu,
                                              const s2a_pyramid* pyr, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && channels > 0, "conv_narrow_pyramid: bad shape");
  S2A_CHECK_ARG(channels % 64 == 0, "conv_narrow_pyramid: channels must be a multiple of 64");
  S2A_CHECK_ARG(out_channels_used >= 1 && out_channels_used <= 16, "conv_narrow_pyramid: 1..16 maps (out_channels_used)");
  // S2A_CONV_NARROW=0: the 64-row launch (A/B switch); it also serves filters too large to stay in LDS
  bool narrow = channels <= kNarrowMaxC;
  if (const char* f = getenv("S2A_CONV_NARROW")) narrow = narrow && atoi(f) != 0;
  if (!narrow)
    return conv3x3_pyramid_impl(x, weight_frag, bias, nullptr, out, ConvExtra{nullptr, nullptr, nullptr, nullptr, 1}, batch,
                                channels, 64, relu, pyr, stream);
  LevelTab lt; int64_t pix = 0;
  const int64_t tiles = build_levels(pyr, batch, &lt, &pix, 8);
  S2A_CHECK_ARG(tiles >= 0, "conv_narrow_pyramid: bad level table (1..8 levels, positive sizes)");
  S2A_CHECK_ARG((uint64_t)pix * channels * 2 < (1ull << 31), "conv_narrow_pyramid: input too large for 32-bit offsets");
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(x && weight_frag && out, "conv_narrow_pyramid: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0 && ((uintptr_t)weight_frag % 16) == 0 &&
                ((uintptr_t)bias % 8) == 0, "conv_narrow_pyramid: tensors must be 16-byte aligned");
  // persistent grid: one workgroup fits a CU (LDS).  S2A_CONV_NARROW_WGS=n caps it (tests: one workgroup walks several levels)
  int64_t grid = std::min<int64_t>(tiles, 256);
  if (const char* f = getenv("S2A_CONV_NARROW_WGS")) grid = std::min<int64_t>(grid, std::max(1, atoi(f)));
  const int lds = narrow_lds_bytes((int)channels);
  auto kern = k_conv3x3_narrow_f16;
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  kern<<<dim3((unsigned)grid), 256, lds, as_stream(stream)>>>((const _Float16*)x, (const _Float16*)weight_frag,
                                                               (const _Float16*)bias, (_Float16*)out, (int)channels,
                                                               (int)out_channels_used, relu,
                                                               (unsigned)((uint64_t)pix * channels * 2), lt, (int)tiles);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
