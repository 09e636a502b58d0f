// Fused ResNet stem for the end-to-end inference config:
//   uint8 image / 255 (val.py:246-247) -> conv 7x7 / stride 2 / pad 3, 3 -> 64 maps with the folded
//   BatchNorm bias -> ReLU -> max-pool 3x3 / stride 2 / pad 1   (models/backbone.py:112-117, :172-175, :307-308)
// as ONE kernel: the [B,64,H/2,W/2] activation (268 MB at batch 8 of 1024^2) and the normalised f16
// image never exist in HBM; traffic is the uint8 image in and the pooled [B,H/4,W/4,64] tile out.
//
// One workgroup = an 8 x 8 tile of pooled outputs = 17 x 17 conv outputs = a 39 x 39 x 3 input
// patch.  The filter lives in registers (fragment order, 88 VGPRs).  The patch is converted once into LDS as f16 (a 256-entry table holds f16(u8 / 255), the
// exact value of the stock f16 division) and the convolution runs on the matrix cores as an
// implicit GEMM: A = filter [64 x K], B = patch columns [K x 289 pixels], K ordered (ky, kx, c) with
// every filter row ky padded from 21 to 24 entries, so that 8 consecutive K entries are 16
// contiguous bytes of one LDS patch row (4-byte aligned: four ds_read_b32 build a B fragment, no
// packing).  K = 7 * 24 = 168 -> 11 MFMA steps of 16 (the tail multiplies zero filter entries).
// Conv tile -> bias + ReLU -> LDS (over the dead patch) -> 3x3 max -> 16-byte stores.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "common.hpp"

namespace s2a {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using h2 = __attribute__((ext_vector_type(2))) _Float16;
using h4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using i16x8 = __attribute__((ext_vector_type(8))) short;

constexpr int kKSteps = 11;                 // 176 = 22 groups of 8 K entries; group q: ky = q / 3, g = q % 3
constexpr int kInRows = 40;                 // 39 patch rows + one zero row for the padded K tail (ky = 7)
constexpr int kInPitch = 136;               // halfs per patch row: 117 used, reads reach index 119
constexpr int kInDw = 31;                   // aligned dwords per patch row (124 bytes from byte -1); a 32nd is carried along unused
constexpr int kConvPitch = 144;             // bytes per staged conv pixel: 64 halfs + 16 B pad
constexpr int kInBytes = kInRows * kInPitch * 2;                    // 10880
constexpr int kConvBytes = 289 * kConvPitch;                        // 41616
constexpr int kStemLds = 640 + 2 * kKSteps * 64 * 16 + (kInBytes > kConvBytes ? kInBytes : kConvBytes);   // table + bias + filter + patch / conv tile
constexpr int kInIters = kInRows / 8;                               // 5 dwords per thread: 8 rows of 32 dwords per pass of the workgroup
static_assert(kInRows % 8 == 0 && 4 * kInDw + 2 < kInPitch, "patch passes");

// filter [64][3][7][7] f16 -> [m 2][step 11][lane 64][8]: lane l, element j =
// W[m*32 + (l & 31)][k = 16*step + 8*(l >> 5) + j], k = ky*24 + kx*3 + c (zero where kx*3+c > 20 or ky > 6)
__global__ void k_stem_pack(const _Float16* __restrict__ w, _Float16* __restrict__ wp) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2 * kKSteps * 64 * 8) return;
  int j = e & 7, lane = (e >> 3) & 63, s = (e >> 9) % kKSteps, m = (e >> 9) / kKSteps;
  int och = m * 32 + (lane & 31);
  int k = 16 * s + 8 * (lane >> 5) + j;
  int ky = k / 24, r = k % 24;
  _Float16 v = (_Float16)0.f;
  if (ky < 7 && r < 21) {
    int kx = r / 3, c = r % 3;
    v = w[((och * 3 + c) * 7 + ky) * 7 + kx];
  }
  wp[e] = v;
}

// Persistent: a workgroup walks tiles blockIdx.x, + gridDim.x, ...  The 22.5 KB of filter fragments go into LDS once
// per workgroup (fetched per tile into every wave's registers they cost 90 KB per tile through the CU's load path and
// 88 VGPRs), and the NEXT tile's patch dwords are requested right after the current patch has been converted, so their
// round trip runs under the MFMA / epilogue / pooling phases of the current tile.
//
// Everything a tile does not need to redo is done once (66 MFMAs per wave and tile stood against 1.6 k vector-ALU
// instructions before this layout; with those halved the LDS array is what binds, docs/HISTORY.md "Round 9"):
//   * what depends on the thread alone (its patch items, its conv pixels, its pooled outputs, the f32 bias of its
//     accumulator rows) is worked out before the tile loop, and a tile's (tx, ty, b) once, when its patch is requested;
//   * `wave` is made provably uniform and every wave runs the same five accumulator units (below), so there is no
//     "this wave has no third pixel tile" exec mask with the accumulators copied round it; the fragments of step
//     s + 1 are read while step s multiplies;
//   * the epilogue rounds a pair, takes the ReLU on the rounded halves (rounding is monotonic and keeps zero, so
//     max(round(v), 0) == round(max(v, 0)); NaN -> 0 either way) and selects once per 8-byte store; the pooling is a
//     packed max (the staged values are never NaN);
//   * a patch dword outside the image becomes 0 before the table (entry 0 is +0), and its four halves leave as
//     b16 + b32 + b16 (index 4d is 4-byte aligned; the patch starts 16 bytes into its buffer so that the half before
//     a row may always be written).
// None of this changes a value: MFMA, K layout, step order per accumulator, table and epilogue roundings are the same.
constexpr int kWBytes = 2 * kKSteps * 64 * 16;                          // 22528
constexpr int kInLead = 16;                                             // bytes in front of the patch (see above)
static_assert(kInLead + kInBytes <= kConvBytes, "the patch lies inside the conv staging buffer");
// kTrain (s2a_stem_u8_f16_train): the same arithmetic up to the rounded pre-activation; then torch's ReLU (a NaN stays a
// NaN) and ATen's max-pool scan, which also leaves sel[b,py,px,o] = 3 dy + dx, the tap the pool took.
template <bool kTrain>
__global__ __launch_bounds__(256, 2) void k_stem(const uint8_t* __restrict__ img,      // [B,H,W,3]
                                                 const _Float16* __restrict__ wp,     // k_stem_pack
                                                 const _Float16* __restrict__ bias,   // [64] or null
                                                 _Float16* __restrict__ out,          // [B,Hp,Wp,64]
                                                 int H, int W, int Hc, int Wc, int Hp, int Wp,
                                                 int tiles_x, int tiles_y, float divisor, int tiles,
                                                 uint8_t* __restrict__ sel) {         // [B,Hp,Wp,64] (kTrain) or null
  extern __shared__ __attribute__((aligned(16))) char smem[];
  _Float16* s_lut = reinterpret_cast<_Float16*>(smem);                 // 256 halfs
  _Float16* s_bias = reinterpret_cast<_Float16*>(smem + 512);          // 64 halfs
  const char* s_w = smem + 640;                                        // filter fragments [m 2][step 11][lane 64] x 16 B
  char* s_conv = smem + 640 + kWBytes;                                 // aliases the patch (dead by then)
  _Float16* s_in = reinterpret_cast<_Float16*>(s_conv + kInLead);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hsel = lane >> 5;
  const int64_t row_bytes = (int64_t)W * 3;

  // ---- per thread, once: its patch dwords (rows pr0 + 8 it, aligned dword pd of the row) and its share of the GEMM.
  // The 10 pixel tiles of 32 (320 >= 289 conv pixels) times the two halves of the 64 maps are 20 units of one 32x32
  // accumulator; every wave takes five: both halves of pixel tiles w and w + 4, and half (w & 1) of pixel tile
  // 8 + (w >> 1).  (Whole pixel tiles per wave made waves 0 and 1 run 66 MFMAs and the other two 44.)
  const int pr0 = tid >> 5, pd = tid & 31;
  const int m3 = wave & 1;
  int ny[3], nx[3];
  bool nok3;                                                   // pixel tile 9 holds pixel 288 alone
  const _Float16 *pbase_n[3], *pbase_w[3];
#pragma unroll
  for (int p = 0; p < 3; p++) {
    int n = (p < 2 ? wave + 4 * p : 8 + (wave >> 1)) * 32 + (lane & 31);
    if (p == 2) nok3 = n < 289;
    n = n < 289 ? n : 0;
    ny[p] = n / 17;
    nx[p] = n - 17 * ny[p];
    const int pbase = (2 * ny[p]) * kInPitch + 6 * nx[p];     // half index of tap (0,0), channel 0
    pbase_n[p] = s_in + pbase + (hsel ? 8 : 0);               // + the upper half's K group: next in the row ...
    pbase_w[p] = s_in + pbase + (hsel ? kInPitch - 16 : 0);   // ... or first of the next row (load_b)
  }

  // patch dwords of a tile: unconditional loads from a clamped address, so none waits for the previous one
  unsigned pv[kInIters];
  bool pok[kInIters];
  const int64_t poff = pr0 * row_bytes + 4 * pd;         // the thread's first dword from the patch's (row 0, dword 0)
  auto patch_issue = [&](int tx, int ty, int b) {
    const int iy0 = 2 * (16 * ty - 1) - 3;               // input origin: row 32*ty - 5
    const int64_t a0 = 96 * (int64_t)tx - 16;            // aligned byte offset inside an image row (x origin = 32*tx - 5 -> byte -15)
    const int64_t bo = a0 + 4 * pd;
    const bool colok = bo >= 0 && bo < row_bytes;
    const int64_t origin = ((int64_t)b * H + iy0) * row_bytes + a0;      // (uniform; may lie in front of the image)
#pragma unroll
    for (int it = 0; it < kInIters; it++) {
      const int r = pr0 + 8 * it, iy = iy0 + r;
      pok[it] = colok && r < 39 && iy >= 0 && iy < H;
      pv[it] = *reinterpret_cast<const unsigned*>(img + (pok[it] ? origin + 8 * it * row_bytes + poff : 0));
    }
  };
  int t = blockIdx.x;
  int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
  patch_issue(tx, ty, b);
  for (int i = tid; i < kWBytes / 16; i += 256)
    *reinterpret_cast<f16x8*>(smem + 640 + i * 16) = *reinterpret_cast<const f16x8*>(wp + i * 8);
  s_lut[tid] = (_Float16)((float)tid / divisor);
  if (tid < 64) s_bias[tid] = bias ? bias[tid] : (_Float16)0.f;
  __syncthreads();
  h4 bq[3][4];                        // accumulator row (rq, e) of map half m = channel 32 m + 8 rq + 4 hsel + e; [2]: half m3
#pragma unroll
  for (int m = 0; m < 3; m++)
#pragma unroll
    for (int rq = 0; rq < 4; rq++)
      bq[m][rq] = *reinterpret_cast<const h4*>(s_bias + (m < 2 ? m : m3) * 32 + 8 * rq + 4 * hsel);

  for (; t < tiles; t += gridDim.x) {
    const int ctx = tx, cty = ty, cb = b;                // this tile; (tx, ty, b) move on to the next one below
    const int cy0 = 16 * cty - 1, cx0 = 16 * ctx - 1;    // conv-output origin of the tile
    __syncthreads();      // the previous tile's pooling has read the conv tile
    _Float16 hv[kInIters][4];
#pragma unroll
    for (int it = 0; it < kInIters; it++) {
      const unsigned v = pok[it] ? pv[it] : 0u;          // outside the image: table entry 0 = +0
#pragma unroll
      for (int e = 0; e < 4; e++) hv[it][e] = s_lut[(v >> (8 * e)) & 255u];
    }
#pragma unroll
    for (int it = 0; it < kInIters; it++) {              // (all gathers first: a store in between would order them)
      _Float16* dst = s_in + (pr0 + 8 * it) * kInPitch + 4 * pd;   // halves 4d-1 .. 4d+2 of the row (byte -15 of the row = index 0)
      dst[-1] = hv[it][0];                               // d = 0: the previous row's unused tail / the lead bytes
      *reinterpret_cast<h2*>(dst) = h2{hv[it][1], hv[it][2]};
      dst[2] = hv[it][3];
    }
    // columns 127..135 of every row are read by nobody (max index 119); nothing to clear
    if (t + (int)gridDim.x < tiles) {                    // next tile's patch: in flight from here on
      const int tn = t + gridDim.x;
      tx = tn % tiles_x, ty = (tn / tiles_x) % tiles_y, b = tn / (tiles_x * tiles_y);
      patch_issue(tx, ty, b);
    }
    __syncthreads();

    // ---- implicit GEMM on the matrix cores, one straight line: acc[2 p + m] = maps 32 m .. of pixel tile p (p < 2),
    // acc[4] = maps 32 m3 .. of the third.  The fragments of step s + 1 are read while step s multiplies.
    f32x16 acc[5];
#pragma unroll
    for (int u = 0; u < 5; u++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[u][r] = 0.f;
    const char* wa_lane = s_w + lane * 16;
    auto load_a = [&](int s, int m) {                    // m == 2: half m3
      return *reinterpret_cast<const f16x8*>(wa_lane + ((m < 2 ? m : m3) * kKSteps + s) * 1024);
    };
    auto load_b = [&](int s, int p) {
      // K group kq = 2 s + hsel of the lane's half: ky = kq / 3, g = kq % 3.  The upper half's group lies 8 halfs
      // behind the lower one's, or at the start of the next patch row when that one is the row's last: two lane-
      // dependent bases per pixel tile, and the step is a constant offset
      const int k0 = 2 * s, koff = (k0 / 3) * kInPitch + 8 * (k0 % 3);
      const unsigned* src = reinterpret_cast<const unsigned*>((k0 % 3 == 2 ? pbase_w[p] : pbase_n[p]) + koff);
      const u32x4 raw = {src[0], src[1], src[2], src[3]};
      return __builtin_bit_cast(f16x8, raw);
    };
    f16x8 wa[2][3], pf[2][3];
#pragma unroll
    for (int k = 0; k < 3; k++) wa[0][k] = load_a(0, k), pf[0][k] = load_b(0, k);
#pragma unroll
    for (int s = 0; s < kKSteps; s++) {
      const int c = s & 1;
      if (s + 1 < kKSteps) {
#pragma unroll
        for (int k = 0; k < 3; k++) wa[c ^ 1][k] = load_a(s + 1, k), pf[c ^ 1][k] = load_b(s + 1, k);
      }
#pragma unroll
      for (int p = 0; p < 2; p++)
#pragma unroll
        for (int m = 0; m < 2; m++)
          acc[2 * p + m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[c][m], pf[c][p], acc[2 * p + m], 0, 0, 0);
      acc[4] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[c][2], pf[c][2], acc[4], 0, 0, 0);
    }
    __syncthreads();                                          // patch dead -> conv staging may overwrite it

    // ---- bias + ReLU -> LDS, zero where the conv pixel lies outside the conv output (the pool's padding:
    // after ReLU every real value is >= 0 and the window always holds its in-range centre, so 0 == -inf here)
    auto stage = [&](const f32x16& a, const h4 (&bh)[4], int p, int m) {
      const int cy = cy0 + ny[p], cx = cx0 + nx[p];
      const bool in = cy >= 0 && cy < Hc && cx >= 0 && cx < Wc;
      char* dst = s_conv + (ny[p] * 17 + nx[p]) * kConvPitch + 8 * hsel + m * 64;
      const h2 zero = {(_Float16)0.f, (_Float16)0.f};
#pragma unroll
      for (int rq = 0; rq < 4; rq++) {
        h2 lo = {(_Float16)(a[rq * 4] + (float)bh[rq][0]), (_Float16)(a[rq * 4 + 1] + (float)bh[rq][1])};
        h2 hi = {(_Float16)(a[rq * 4 + 2] + (float)bh[rq][2]), (_Float16)(a[rq * 4 + 3] + (float)bh[rq][3])};
        const h2 plo = lo, phi = hi;
        lo = __builtin_elementwise_max(lo, zero);
        hi = __builtin_elementwise_max(hi, zero);
        if constexpr (kTrain) {                                 // the max above answers 0 for a NaN: put it back
          lo = h2{plo[0] != plo[0] ? plo[0] : lo[0], plo[1] != plo[1] ? plo[1] : lo[1]};
          hi = h2{phi[0] != phi[0] ? phi[0] : hi[0], phi[1] != phi[1] ? phi[1] : hi[1]};
        }
        const h4 v4 = {lo[0], lo[1], hi[0], hi[1]};
        *reinterpret_cast<h4*>(dst + 16 * rq) = in ? v4 : h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
      }
    };
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int m = 0; m < 2; m++) stage(acc[2 * p + m], bq[m], p, m);
    if (nok3) stage(acc[4], bq[2], 2, m3);
    __syncthreads();

    // ---- 3x3 / stride 2 max over the staged conv tile, 8 channels (16 B) per item
#pragma unroll
    for (int it = 0; it < 2; it++) {
      const int item = tid + 256 * it, pp = item >> 3, cg = item & 7;
      const int py = pp >> 3, px = pp & 7;
      const int oy = 8 * cty + py, ox = 8 * ctx + px;
      const char* win = s_conv + ((2 * py) * 17 + 2 * px) * kConvPitch + cg * 16;
      if constexpr (kTrain) {
        // ATen's scan (max_pool2d_with_indices): dy then dx over the taps inside the conv map, starting from -inf at the
        // first of them; a later tap takes over only if it is greater or NaN.  A staged pixel outside the map is never read
        const int dy0 = oy == 0 ? 1 : 0, dx0 = ox == 0 ? 1 : 0;
        f16x8 best;
        unsigned char id[8];
#pragma unroll
        for (int e = 0; e < 8; e++) best[e] = -(_Float16)__builtin_inff(), id[e] = (unsigned char)(3 * dy0 + dx0);
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
          for (int dx = 0; dx < 3; dx++) {
            const int cy = 2 * oy - 1 + dy, cx = 2 * ox - 1 + dx;
            if (!(cy >= 0 && cy < Hc && cx >= 0 && cx < Wc)) continue;
            const f16x8 v = *reinterpret_cast<const f16x8*>(win + (dy * 17 + dx) * kConvPitch);
#pragma unroll
            for (int e = 0; e < 8; e++)
              if (v[e] > best[e] || v[e] != v[e]) best[e] = v[e], id[e] = (unsigned char)(3 * dy + dx);
          }
        if (oy < Hp && ox < Wp) {
          const int64_t o = (((int64_t)cb * Hp + oy) * Wp + ox) * 64 + cg * 8;
          *reinterpret_cast<f16x8*>(out + o) = best;
          uint2 packed = {0u, 0u};
#pragma unroll
          for (int e = 0; e < 4; e++) packed.x |= (unsigned)id[e] << (8 * e), packed.y |= (unsigned)id[4 + e] << (8 * e);
          *reinterpret_cast<uint2*>(sel + o) = packed;
        }
      } else {
        // the staged halves are >= +0 and never NaN (ReLU above), so their order as 16-bit integers is their order
        // as numbers: a packed integer max, which unlike the f16 one needs no canonicalised operands
        i16x8 mx = *reinterpret_cast<const i16x8*>(win);
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
          for (int dx = 0; dx < 3; dx++) {
            if (dy == 0 && dx == 0) continue;
            mx = __builtin_elementwise_max(mx, *reinterpret_cast<const i16x8*>(win + (dy * 17 + dx) * kConvPitch));
          }
        if (oy < Hp && ox < Wp)
          *reinterpret_cast<i16x8*>(out + (((int64_t)cb * Hp + oy) * Wp + ox) * 64 + cg * 8) = mx;
      }
    }
  }
}

// ---- backward of the training stem (s2a_stem_backward_f16): filter and bias gradient, no input gradient.
// One workgroup = one slice: it walks the forward's tiles s, s + slices, ... (8 x 8 pooled windows each) and keeps the whole
// [64 maps] x [147 filter taps + the bias column] gradient in its accumulators until the last tile.  Per tile the patch is
// staged through the table exactly as in the forward, and the gradient is contracted on the matrix cores with
//   K = (window, pool tap) = 64 x 9:  A[o][k] = the window's grad_out[o] where the pool took this tap and the ReLU passed
//                                              (SELECTED, else +0: a masked inf or NaN never meets a product),
//                                     B[k][t] = the patch value under filter tap t of the conv pixel this pool tap names,
// so every product is one term of the definition, exact in f32, and no gradient is rounded on the way.  Column 147 of B is
// 1 (the bias sum), columns 148 .. 159 are 0.  Wave w takes the windows of pooled rows 2 w and 2 w + 1 (a quarter of K); the
// four waves' sums are added in wave order at the end.  t = (c * 7 + ky) * 7 + kx: the gradient's own order.
constexpr int kGradTaps = 147;
constexpr int kGradCols = 64 * kGradTaps + 64;      // floats per slice
constexpr int kBwdMaxSlices = 256;
constexpr int kGoPitch = 72;                        // halfs per map of the transposed grad_out tile (64 windows + pad)
constexpr int kSelPitch = 72;                       // bytes per map of the transposed tap tile
constexpr int kBwdInOff = 512;                      // table in front
constexpr int kBwdGoOff = 11520;                    // >= kBwdInOff + kInLead + kInBytes
constexpr int kBwdSelOff = kBwdGoOff + 64 * kGoPitch * 2;
constexpr int kBwdStage = kBwdSelOff + 64 * kSelPitch;
constexpr int kBwdRed = 10 * 16 * 64 * 4;           // one wave's accumulators
constexpr int kBwdLds = kBwdRed > kBwdStage ? kBwdRed : kBwdStage;
static_assert(kBwdInOff + kInLead + kInBytes <= kBwdGoOff && kBwdLds <= 65536, "backward LDS layout");

__global__ __launch_bounds__(256, 1) void k_stem_bwd(const uint8_t* __restrict__ img,        // [B,H,W,3]
                                                     const _Float16* __restrict__ out,       // [B,Hp,Wp,64] forward output
                                                     const uint8_t* __restrict__ sel,        // [B,Hp,Wp,64] pool taps
                                                     const _Float16* __restrict__ gout,      // [B,Hp,Wp,64]
                                                     float* __restrict__ partial,            // [slices][kGradCols]
                                                     int H, int W, int Hp, int Wp, int tiles_x, int tiles_y,
                                                     float divisor, int tiles) {
  __shared__ __attribute__((aligned(16))) char smem[kBwdLds];
  _Float16* s_lut = reinterpret_cast<_Float16*>(smem);
  _Float16* s_in = reinterpret_cast<_Float16*>(smem + kBwdInOff + kInLead);
  _Float16* s_go = reinterpret_cast<_Float16*>(smem + kBwdGoOff);
  uint8_t* s_sel = reinterpret_cast<uint8_t*>(smem + kBwdSelOff);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hsel = lane >> 5;
  const int64_t row_bytes = (int64_t)W * 3;

  // the tile's inputs, requested one tile ahead: patch dwords as in k_stem, and 16 maps of one window per thread
  const int pr0 = tid >> 5, pd = tid & 31;
  const int win = tid >> 2, cg = tid & 3, lpy = win >> 3, lpx = win & 7;
  unsigned pv[kInIters];
  bool pok[kInIters], wok;
  f16x8 gv[2], ov[2];
  u32x4 sv;
  const int64_t poff = pr0 * row_bytes + 4 * pd;
  auto issue = [&](int tx, int ty, int b) {
    const int iy0 = 2 * (16 * ty - 1) - 3;
    const int64_t a0 = 96 * (int64_t)tx - 16;
    const int64_t bo = a0 + 4 * pd;
    const bool colok = bo >= 0 && bo < row_bytes;
    const int64_t origin = ((int64_t)b * H + iy0) * row_bytes + a0;
#pragma unroll
    for (int it = 0; it < kInIters; it++) {
      const int rr = pr0 + 8 * it, iy = iy0 + rr;
      pok[it] = colok && rr < 39 && iy >= 0 && iy < H;
      pv[it] = *reinterpret_cast<const unsigned*>(img + (pok[it] ? origin + 8 * it * row_bytes + poff : 0));
    }
    const int oy = 8 * ty + lpy, ox = 8 * tx + lpx;
    wok = oy < Hp && ox < Wp;
    const int64_t o = wok ? (((int64_t)b * Hp + oy) * Wp + ox) * 64 + 16 * cg : 0;   // (a window outside the map: any valid address)
#pragma unroll
    for (int q = 0; q < 2; q++) {
      gv[q] = *reinterpret_cast<const f16x8*>(gout + o + 8 * q);
      ov[q] = *reinterpret_cast<const f16x8*>(out + o + 8 * q);
    }
    sv = *reinterpret_cast<const u32x4*>(sel + o);
  };

  // per lane, once: where filter tap t = 32 nt + r of its B columns starts in the patch, from the lane's first window row
  const _Float16* pbase[5];
#pragma unroll
  for (int nt = 0; nt < 5; nt++) {
    const int t = 32 * nt + r;
    const int c = t / 49, ky = (t % 49) / 7, kx = t % 7;
    pbase[nt] = s_in + (t < kGradTaps ? ky * kInPitch + kx * 3 + c : 0) + 4 * (2 * wave + hsel) * kInPitch;
  }
  const bool real4 = 128 + r < kGradTaps, one4 = 128 + r == kGradTaps;

  f32x16 acc[2][5];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int nt = 0; nt < 5; nt++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[m][nt][i] = 0.f;

  int t = blockIdx.x;
  if (t < tiles) issue(t % tiles_x, (t / tiles_x) % tiles_y, t / (tiles_x * tiles_y));
  s_lut[tid] = (_Float16)((float)tid / divisor);
  for (; t < tiles; t += gridDim.x) {
    __syncthreads();                  // the table is there / the previous tile's fragments have been read
    {
      _Float16 hv[kInIters][4];
#pragma unroll
      for (int it = 0; it < kInIters; it++) {
        const unsigned v = pok[it] ? pv[it] : 0u;
#pragma unroll
        for (int e = 0; e < 4; e++) hv[it][e] = s_lut[(v >> (8 * e)) & 255u];
      }
#pragma unroll
      for (int it = 0; it < kInIters; it++) {
        _Float16* dst = s_in + (pr0 + 8 * it) * kInPitch + 4 * pd;
        dst[-1] = hv[it][0];
        *reinterpret_cast<h2*>(dst) = h2{hv[it][1], hv[it][2]};
        dst[2] = hv[it][3];
      }
      // the window's 16 maps, transposed to [map][window]; tap 255 (no tap) where the window lies outside the map or the
      // ReLU did not pass (out <= 0; a NaN output passes, as in s2a_conv_backward_prep_f16)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int o = 16 * cg + e;
        const _Float16 ovv = ov[e >> 3][e & 7];
        const unsigned tap = (sv[e >> 2] >> (8 * (e & 3))) & 255u;
        s_go[o * kGoPitch + win] = gv[e >> 3][e & 7];
        s_sel[o * kSelPitch + win] = (uint8_t)((wok && !(ovv <= (_Float16)0.f)) ? tap : 255u);
      }
    }
    if (t + (int)gridDim.x < tiles) {
      const int tn = t + gridDim.x;
      issue(tn % tiles_x, (tn / tiles_x) % tiles_y, tn / (tiles_x * tiles_y));
    }
    __syncthreads();

    f16x8 gof[2];
    uint2 self[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      gof[m] = *reinterpret_cast<const f16x8*>(s_go + (32 * m + r) * kGoPitch + 16 * wave + 8 * hsel);
      self[m] = *reinterpret_cast<const uint2*>(s_sel + (32 * m + r) * kSelPitch + 16 * wave + 8 * hsel);
    }
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
      const int dy = tap / 3, dx = tap % 3;
      f16x8 a[2], bf[5];
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const unsigned sj = ((j < 4 ? self[m].x : self[m].y) >> (8 * (j & 3))) & 255u;
          a[m][j] = sj == (unsigned)tap ? gof[m][j] : (_Float16)0.f;
        }
#pragma unroll
      for (int nt = 0; nt < 5; nt++) {
        const _Float16* src = pbase[nt] + 2 * dy * kInPitch + 6 * dx;      // window lpx = j: 12 halfs further each
#pragma unroll
        for (int j = 0; j < 8; j++) bf[nt][j] = src[12 * j];
      }
#pragma unroll
      for (int j = 0; j < 8; j++) bf[4][j] = real4 ? bf[4][j] : (one4 ? (_Float16)1.f : (_Float16)0.f);
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int nt = 0; nt < 5; nt++)
          acc[m][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m], bf[nt], acc[m][nt], 0, 0, 0);
    }
  }

  // ---- the four waves' sums, ((w0 + w1) + w2) + w3, through LDS (over the dead staging buffers)
  float* red = reinterpret_cast<float*>(smem);
  for (int ww = 1; ww < 4; ww++) {
    __syncthreads();
    if (wave == ww) {
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int nt = 0; nt < 5; nt++)
#pragma unroll
          for (int i = 0; i < 16; i++) red[((m * 5 + nt) * 16 + i) * 64 + lane] = acc[m][nt][i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int m = 0; m < 2; m++)
#pragma unroll
        for (int nt = 0; nt < 5; nt++)
#pragma unroll
          for (int i = 0; i < 16; i++) acc[m][nt][i] += red[((m * 5 + nt) * 16 + i) * 64 + lane];
    }
  }
  if (wave == 0) {
    float* dst = partial + (int64_t)blockIdx.x * kGradCols;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
      for (int nt = 0; nt < 5; nt++) {
        const int tt = 32 * nt + r;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const int o = 32 * m + (i & 3) + 8 * (i >> 2) + 4 * hsel;      // accumulator row of the 32 x 32 tile
          if (tt < kGradTaps) dst[o * kGradTaps + tt] = acc[m][nt][i];
          else if (tt == kGradTaps) dst[64 * kGradTaps + o] = acc[m][nt][i];
        }
      }
  }
}

// what is wrong with a stem problem, or nullptr: the checks the entry points and the slices query share
const char* stem_shape_problem(int64_t batch, int64_t height, int64_t width) {
  if (!(batch >= 0 && height >= 7 && width >= 7)) return "bad shape";
  if (width % 4 != 0) return "image width must be a multiple of 4 (aligned 32-bit loads of RGB rows)";
  if (!(height < (1ll << 24) && width < (1ll << 24) && batch < (1ll << 31) && batch * height * width * 3 < (1ll << 40)))
    return "image too large";
  return nullptr;
}

struct StemGeom {
  int H, W, Hc, Wc, Hp, Wp, tiles_x, tiles_y;
  int64_t tiles;
};
StemGeom stem_geom(int64_t batch, int64_t height, int64_t width) {
  StemGeom q;
  q.H = (int)height, q.W = (int)width;
  q.Hc = (q.H - 1) / 2 + 1, q.Wc = (q.W - 1) / 2 + 1;          // 7x7 / 2 / pad 3
  q.Hp = (q.Hc - 1) / 2 + 1, q.Wp = (q.Wc - 1) / 2 + 1;        // 3x3 / 2 / pad 1
  q.tiles_x = (q.Wp + 7) / 8, q.tiles_y = (q.Hp + 7) / 8;
  q.tiles = batch * q.tiles_x * q.tiles_y;
  return q;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" int s2a_stem_pack_weight_f16(const void* weight, void* packed, s2a_stream_t stream) {
  S2A_CHECK_ARG(weight && packed, "stem_pack_weight: NULL tensor");
  const int total = 2 * kKSteps * 64 * 8;
  k_stem_pack<<<(total + 255) / 256, 256, 0, as_stream(stream)>>>((const _Float16*)weight, (_Float16*)packed);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int64_t s2a_stem_packed_elems(void) { return 2 * kKSteps * 64 * 8; }

namespace {
// both forwards: s2a_stem_u8_f16 (sel == nullptr, train == false) and s2a_stem_u8_f16_train
int stem_forward(const char* who, bool train, const void* image_u8, const void* weight_packed, const void* bias, void* out,
                 void* sel, int64_t batch, int64_t height, int64_t width, float divisor, s2a_stream_t stream) {
  S2A_CHECK_ARG(batch >= 0 && height >= 7 && width >= 7, "%s: bad shape", who);
  S2A_CHECK_ARG(width % 4 == 0, "%s: image width must be a multiple of 4 (aligned 32-bit loads of RGB rows)", who);
  S2A_CHECK_ARG(divisor > 0, "%s: divisor must be positive", who);
  S2A_CHECK_ARG(batch * height * width * 3 < (1ll << 40), "%s: image too large", who);
  if (batch == 0) return S2A_OK;
  S2A_CHECK_ARG(image_u8 && weight_packed && out && (sel || !train), "%s: NULL tensor", who);
  S2A_CHECK_ARG(((uintptr_t)image_u8 % 4) == 0 && ((uintptr_t)weight_packed % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                ((uintptr_t)bias % 2) == 0 && ((uintptr_t)sel % 8) == 0, "%s: misaligned tensor", who);
  const StemGeom q = stem_geom(batch, height, width);
  S2A_CHECK_ARG(q.tiles < (1ll << 31), "%s: too many tiles", who);
  auto kern = train ? k_stem<true> : k_stem<false>;
  S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kStemLds));
  // persistent grid: two workgroups fit a CU (LDS)
  const unsigned grid = (unsigned)std::min<int64_t>(q.tiles, 256 * 2);
  kern<<<grid, 256, kStemLds, as_stream(stream)>>>((const uint8_t*)image_u8, (const _Float16*)weight_packed,
                                                    (const _Float16*)bias, (_Float16*)out, q.H, q.W, q.Hc, q.Wc, q.Hp,
                                                    q.Wp, q.tiles_x, q.tiles_y, divisor, (int)q.tiles, (uint8_t*)sel);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
}  // namespace

extern "C" int s2a_stem_u8_f16(const void* image_u8, const void* weight_packed, const void* bias, void* out,
                               int64_t batch, int64_t height, int64_t width, float divisor,
                               s2a_stream_t stream) {
  return stem_forward("stem", false, image_u8, weight_packed, bias, out, nullptr, batch, height, width, divisor, stream);
}

extern "C" int s2a_stem_u8_f16_train(const void* image_u8, const void* weight_packed, const void* bias, void* out, void* sel,
                                     int64_t batch, int64_t height, int64_t width, float divisor, s2a_stream_t stream) {
  return stem_forward("stem_train", true, image_u8, weight_packed, bias, out, sel, batch, height, width, divisor, stream);
}

extern "C" int s2a_stem_backward_slices(int64_t batch, int64_t height, int64_t width) {
  if (stem_shape_problem(batch, height, width) || batch == 0) return 0;
  const StemGeom q = stem_geom(batch, height, width);
  if (q.tiles >= (1ll << 31)) return 0;
  return (int)std::min<int64_t>(q.tiles, kBwdMaxSlices);      // (shapes only)
}

extern "C" int s2a_stem_backward_f16(const void* image_u8, const void* out, const void* sel, const void* grad_out,
                                     void* partial, int slices, int64_t batch, int64_t height, int64_t width,
                                     float divisor, s2a_stream_t stream) {
  const char* problem = stem_shape_problem(batch, height, width);
  S2A_CHECK_ARG(!problem, "stem_backward: %s", problem);
  S2A_CHECK_ARG(batch > 0, "stem_backward: bad shape (an empty batch has no slices)");
  S2A_CHECK_ARG(divisor > 0, "stem_backward: divisor must be positive");
  const StemGeom q = stem_geom(batch, height, width);
  S2A_CHECK_ARG(q.tiles < (1ll << 31), "stem_backward: too many tiles");
  const int want = s2a_stem_backward_slices(batch, height, width);
  S2A_CHECK_ARG(slices == want, "stem_backward: slices is %d, s2a_stem_backward_slices answers %d", slices, want);
  S2A_CHECK_ARG(image_u8 && out && sel && grad_out && partial, "stem_backward: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)image_u8 % 4) == 0 && aligned16(out) && aligned16(sel) && aligned16(grad_out) && aligned16(partial),
                "stem_backward: misaligned tensor (the image 4 bytes, everything else 16)");
  k_stem_bwd<<<(unsigned)slices, 256, 0, as_stream(stream)>>>((const uint8_t*)image_u8, (const _Float16*)out,
                                                              (const uint8_t*)sel, (const _Float16*)grad_out, (float*)partial,
                                                              q.H, q.W, q.Hp, q.Wp, q.tiles_x, q.tiles_y, divisor, (int)q.tiles);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
