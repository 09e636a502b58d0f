// Training augmentation of the reference's S2ANet recipe (data/hyps/hyp.scratch.s2anet.yaml: degrees 180, fliplr 0.5,
// everything else 0) on the device: utils/augmentations.py:93-175 (random_perspective_rotation with scale = shear =
// translate = perspective = 0) and utils/datasets_rotation.py:480-492 (np.flipud, np.fliplr), then poly_to_rotated_box_np.
//
//   k_augment_draw    one workgroup: Philox4x32-10 per image -> params int32 [B,4] = (rot, flipud, fliplr, 0); step += 1
//   k_augment_images  one workgroup per 64 x 64 destination tile of one image: the source tile (the same pixels for the
//                     four non-transposing elements, the transposed tile for the other four) comes in along rows in dwords,
//                     waits in the LDS, and leaves along rows as three dwords per four pixels; border pixels included
//   k_augment_labels  one thread per label row, float64 (augment_geom.hpp)
// Nothing is allocated, nothing is read back, every launch is on the caller's stream.
#include "common.hpp"

#include "augment_geom.hpp"

namespace s2a {
namespace {

constexpr int kThreads = 256;
using aug::kPitch;
using aug::kTile;
constexpr int kRowsPerWave = kTile / (kThreads / 64);

struct __attribute__((packed, aligned(4))) Dword3 {
  uint32_t a, b, c;
};

__global__ __launch_bounds__(1024) void k_augment_draw(int64_t* __restrict__ step, const int64_t* __restrict__ seed,
                                                       int batch, int turn, float p_ud, float p_lr,
                                                       int32_t* __restrict__ params) {
  const uint64_t s = (uint64_t)step[0], key = (uint64_t)seed[0];
  for (int b = threadIdx.x; b < batch; b += blockDim.x) {
    int32_t p[4];
    aug::draw_params((uint32_t)b, s, key, turn, p_ud, p_lr, p);
    *reinterpret_cast<int4*>(params + 4 * (int64_t)b) = make_int4(p[0], p[1], p[2], p[3]);
  }
  __syncthreads();   // every thread has read step
  if (threadIdx.x == 0) step[0] = (int64_t)(s + 1);
}

__global__ __launch_bounds__(kThreads) void k_augment_images(const uint8_t* __restrict__ src,
                                                             const int32_t* __restrict__ params, int S,
                                                             uint8_t* __restrict__ dst) {
  __shared__ uint32_t tile[kTile * kPitch];
  const int b = blockIdx.z;
  const int X0 = blockIdx.x * kTile, Y0 = blockIdx.y * kTile;
  const int4 prm = *reinterpret_cast<const int4*>(params + 4 * (int64_t)b);   // uniform: a workgroup is inside one image
  const aug::TilePlan p = aug::tile_plan(prm.x, prm.y != 0, prm.z != 0, S, X0, Y0);
  const int64_t row_dwords = (int64_t)3 * S / 4;
  const uint32_t* src32 = reinterpret_cast<const uint32_t*>(src) + (int64_t)b * S * row_dwords;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t v[kRowsPerWave];
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++) {
    const int r = wave * kRowsPerWave + i, sy = p.sy_lo + r;
    v[i] = (r < p.nv && sy < S && lane < p.ndw) ? src32[(int64_t)sy * row_dwords + p.d0 + lane] : 0u;
  }
#pragma unroll
  for (int i = 0; i < kRowsPerWave; i++)
    if (lane < kPitch) tile[(wave * kRowsPerWave + i) * kPitch + lane] = v[i];
  __syncthreads();

  // four destination pixels (three dwords) per lane and step.  Lanes 0-7 and 32-39 share a destination row: within one
  // half-wave, eight pixel groups of four rows
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(tile);
  uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst) + (int64_t)b * S * row_dwords;
  const int g = (lane & 7) | ((lane >> 5) << 3), ry = (lane >> 3) & 3;
  if (4 * g >= p.tw) return;
  for (int yy = wave * 4 + ry; yy < p.th; yy += 16) {
    const int Y = Y0 + yy;
    uint32_t px[4], o[3];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int src_at = aug::tile_source_byte(p, S, X0 + 4 * g + j, Y);
      const int at = src_at < 0 ? 0 : src_at;
      const uint32_t v3 = (uint32_t)bytes[at] | ((uint32_t)bytes[at + 1] << 8) | ((uint32_t)bytes[at + 2] << 16);
      px[j] = src_at < 0 ? (uint32_t)(aug::kBorder * 0x010101) : v3;
    }
    aug::pack_pixels(px, o);
    *reinterpret_cast<Dword3*>(dst32 + (int64_t)Y * row_dwords + ((3 * (X0 + 4 * g)) >> 2)) = Dword3{o[0], o[1], o[2]};
  }
}

__global__ __launch_bounds__(kThreads) void k_augment_status_clear(int64_t* __restrict__ status) {
  if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kThreads) void k_augment_labels(const float* __restrict__ labels, int64_t n_rows,
                                                             const int32_t* __restrict__ params, int batch, int S,
                                                             int normalize, float* __restrict__ targets,
                                                             int64_t* __restrict__ status) {
  __shared__ int counts[4];
  if (threadIdx.x < 4) counts[threadIdx.x] = 0;
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (g < n_rows) {
    const float* row = labels + g * 10;
    float* t = targets + g * 7;
    const float img_f = row[0];
    const bool real = img_f >= 0.0f && img_f < (float)batch;   // NaN: padding
    int fate = aug::kPadding;
    aug::RBox box = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (real) {
      const int4 prm = *reinterpret_cast<const int4*>(params + 4 * (int64_t)(int)img_f);
      double pts[8];
#pragma unroll
      for (int i = 0; i < 8; i++) pts[i] = (double)row[2 + i];
      fate = aug::augment_label(pts, prm.x, prm.y != 0, prm.z != 0, (double)S, box);
    }
    if (fate == aug::kKept) {
      const double div = normalize ? (double)S : 1.0;   // xywhtheta2xywhtheta_n: x, w by the width, y, h by the height
      t[0] = (float)(int)img_f;
      t[1] = row[1];
      t[2] = (float)(box.cx / div);
      t[3] = (float)(box.cy / div);
      t[4] = (float)(box.w / div);
      t[5] = (float)(box.h / div);
      t[6] = (float)box.theta;
    } else {
      t[0] = -1.0f;
#pragma unroll
      for (int i = 1; i < 7; i++) t[i] = 0.0f;
    }
    if (real) {
      atomicAdd(&counts[0], 1);
      atomicAdd(&counts[fate == aug::kKept ? 1 : fate == aug::kOffCentre ? 2 : 3], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && counts[threadIdx.x] != 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(status) + threadIdx.x, (unsigned long long)counts[threadIdx.x]);
}

bool bad_prob(float p) { return !(p >= 0.0f && p <= 1.0f); }

}  // namespace
}  // namespace s2a

extern "C" int s2a_augment_draw(int64_t* step, const int64_t* seed, int64_t batch, int turn, float p_flipud, float p_fliplr,
                                int32_t* params, s2a_stream_t stream) {
  using namespace s2a;
  S2A_CHECK_ARG(step != nullptr && seed != nullptr && params != nullptr, "s2a_augment_draw: NULL step / seed / params");
  S2A_CHECK_ARG(batch > 0 && batch <= (1 << 24), "s2a_augment_draw: batch must be 1 to 2^24 (got %lld)", (long long)batch);
  S2A_CHECK_ARG(!bad_prob(p_flipud) && !bad_prob(p_fliplr), "s2a_augment_draw: flip probabilities must lie in [0, 1] (got %g, %g)",
                (double)p_flipud, (double)p_fliplr);
  S2A_CHECK_ARG(((uintptr_t)params & 15u) == 0 && ((uintptr_t)step & 7u) == 0 && ((uintptr_t)seed & 7u) == 0,
                "s2a_augment_draw: params must be 16-byte aligned, step and seed 8-byte aligned");
  const int threads = batch >= 1024 ? 1024 : (int)((batch + 63) / 64 * 64);
  k_augment_draw<<<1, threads, 0, as_stream(stream)>>>(step, seed, (int)batch, turn != 0, p_flipud, p_fliplr, params);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_augment_images_u8(const uint8_t* src, const int32_t* params, int64_t batch, int64_t height, int64_t width,
                                     uint8_t* dst, s2a_stream_t stream) {
  using namespace s2a;
  S2A_CHECK_ARG(src != nullptr && params != nullptr && dst != nullptr, "s2a_augment_images_u8: NULL src / params / dst");
  S2A_CHECK_ARG(batch > 0 && height > 0 && width > 0, "s2a_augment_images_u8: sizes must be positive (batch %lld, %lld x %lld)",
                (long long)batch, (long long)height, (long long)width);
  S2A_CHECK_ARG(height == width, "s2a_augment_images_u8: chips must be square (got %lld x %lld)", (long long)height, (long long)width);
  S2A_CHECK_ARG(width % 4 == 0 && width >= 8 && width <= 32768,
                "s2a_augment_images_u8: width must be a multiple of 4 in [8, 32768] (got %lld)", (long long)width);
  S2A_CHECK_ARG(batch <= 65535, "s2a_augment_images_u8: batch out of range (%lld > 65535)", (long long)batch);
  S2A_CHECK_ARG((((uintptr_t)src | (uintptr_t)dst) & 3u) == 0 && ((uintptr_t)params & 15u) == 0,
                "s2a_augment_images_u8: src and dst must be 4-byte aligned, params 16-byte aligned");
  const uintptr_t bytes = (uintptr_t)batch * (uintptr_t)height * (uintptr_t)width * 3u;
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  S2A_CHECK_ARG(s0 + bytes <= d0 || d0 + bytes <= s0, "s2a_augment_images_u8: src and dst overlap (the map is not in place)");
  const unsigned tiles = (unsigned)((width + kTile - 1) / kTile);
  k_augment_images<<<dim3(tiles, tiles, (unsigned)batch), kThreads, 0, as_stream(stream)>>>(src, params, (int)width, dst);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_augment_labels(const float* labels, int64_t n_rows, const int32_t* params, int64_t batch, int64_t height,
                                  int64_t width, int normalize, float* targets, int64_t* status, s2a_stream_t stream) {
  using namespace s2a;
  S2A_CHECK_ARG(labels != nullptr && params != nullptr && targets != nullptr && status != nullptr,
                "s2a_augment_labels: NULL labels / params / targets / status");
  S2A_CHECK_ARG(n_rows > 0 && batch > 0 && height > 0 && width > 0,
                "s2a_augment_labels: sizes must be positive (rows %lld, batch %lld, %lld x %lld)", (long long)n_rows,
                (long long)batch, (long long)height, (long long)width);
  S2A_CHECK_ARG(height == width, "s2a_augment_labels: chips must be square (got %lld x %lld)", (long long)height, (long long)width);
  S2A_CHECK_ARG(width % 4 == 0 && width <= 32768, "s2a_augment_labels: width must be a multiple of 4 up to 32768 (got %lld)",
                (long long)width);
  S2A_CHECK_ARG(batch <= (1 << 24) && n_rows <= ((int64_t)1 << 31) * kThreads - 1, "s2a_augment_labels: batch or rows out of range");
  S2A_CHECK_ARG(((uintptr_t)params & 15u) == 0 && ((uintptr_t)status & 7u) == 0 && (((uintptr_t)labels | (uintptr_t)targets) & 3u) == 0,
                "s2a_augment_labels: params must be 16-byte aligned, status 8-byte, labels and targets 4-byte");
  hipStream_t st = as_stream(stream);
  k_augment_status_clear<<<1, kThreads, 0, st>>>(status);
  k_augment_labels<<<(unsigned)((n_rows + kThreads - 1) / kThreads), kThreads, 0, st>>>(labels, n_rows, params, (int)batch, (int)width,
                                                                                        normalize != 0, targets, status);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
