// Rotated-box IoU for MI355X (gfx950, wave64): the [N,M] matrix (s2a_box_iou_rotated) and the pairwise form
// (s2a_box_iou_rotated_pairs).
// COMPILE WITH -ffp-contract=off (see rbox_geom.hpp).
//
// Replaces the reference's CUDA extension:
//   utils/box_iou_rotated/src/box_iou_rotated_cuda.cu:14-101
//
// MI355X-first structure (not the reference's one-thread-per-pair tiles):
//   1. per-box pre-pass: double cos/sin once per box (PreBox), not once per pair
//   2. CULL pass: every pair gets a 10-instruction circumscribed-circle test that is
//      provably exact (culled => the reference returns exactly 0.0f).  Surviving pairs
//      (~1 % of random DOTA-like boxes) are compacted — LDS queue per workgroup, one
//      global atomic per flush — into a dense pair list
//   3. HEAVY pass: the divergent, register-hungry clipping/hull code runs on the dense
//      list with all 64 lanes busy; its <=24 candidate points sit in LDS ([point][thread]
//      float2, conflict-free) instead of scratch
//   4. large outputs: the zero fill of the matrix runs PACED on a side stream beside 2 and 3, and a scatter drops the
//      values into place after the join (side_set: the registry of rotated_ops.hip, through common.hpp)
// The NMS (rotated_ops.hip) runs the same three steps on its own tiles; what the two share is rotated_common.hpp.
// Consumers inside the library: the matrix form of s2a_assign_labels (assign_ops.hip), through the public header.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "common.hpp"
#include "rbox_geom.hpp"
#include "rotated_common.hpp"

namespace s2a {
namespace {

constexpr uint32_t kIouRedo = 0x7fc5a5a5u;   // marker of a pair that needs all 24 slots

// ---------------------------------------------------------------- pre-pass
// both box sets of box_iou_rotated in one launch; the first threads also reset the per-chunk pair counters
__global__ void k_prep_boxes2(const float* __restrict__ b1, int64_t n, PreBox* __restrict__ o1,
                              const float* __restrict__ b2, int64_t m, PreBox* __restrict__ o2,
                              unsigned long long* __restrict__ counters, int ncounters) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncounters) counters[i] = 0ull;
  if (i < n) {
    const float* b = b1 + 5 * i;
    o1[i] = make_prebox(b[0], b[1], b[2], b[3], b[4], 0.f);
  } else if (i < n + m) {
    const float* b = b2 + 5 * (i - n);
    o2[i - n] = make_prebox(b[0], b[1], b[2], b[3], b[4], 0.f);
  }
}

// ================================================================= box_iou_rotated
// CULL: workgroup = 1024 columns (4 per lane: one 16-byte store per lane per row) x up to 64 rows.
// Every element of the tile is stored here as 0.0f -- exact for culled pairs; the ~1 % that survive
// the cull are also queued and overwritten by the heavy pass (same stream, later kernel).  Row boxes
// are staged in LDS and read one iteration ahead so no row waits on a load.  HBM-write-bound, so the
// kernel keeps its LDS small (18 KB: eight workgroups = 32 waves per CU; the first version staged the column
// boxes as well, 76 KB = two workgroups per CU, and reached a quarter of the write bandwidth).
// Queue discipline: every decision that all threads must take alike is taken through __syncthreads_or -- a
// plain read of an LDS counter after a barrier is NOT uniform (a fast wave may already be pushing again).
constexpr int kIouRowsPerWg = 64;
constexpr int kIouQueue = 1024;      // LDS pair queue (survivors of BOTH tests); a drain batch adds <= 256
constexpr int kIouQ1 = 3072;         // first-stage queue: circle-test survivors, (row << 10 | column) per entry
constexpr int kIouQ1DrainAt = 1024;  // <= 2048 pushes per two rows on top of this

template <bool STORE>
__global__ __launch_bounds__(kThreads) void k_iou_cull(const PreBox* __restrict__ P1,
                                                       const PreBox* __restrict__ P2,
                                                       int64_t row0, int64_t row1, int64_t m,
                                                       float* __restrict__ out,
                                                       uint2* __restrict__ gq,
                                                       unsigned long long* __restrict__ gcount,
                                                       unsigned long long cap) {
  __shared__ uint2 s_q[kIouQueue];
  __shared__ unsigned s_count, s_base[2], s_cnt1;
  __shared__ PreBox s_rows[kIouRowsPerWg];
  __shared__ unsigned short s_q1[kIouQ1];
  PairQueue Q{s_q, &s_count, s_base};
  if (threadIdx.x == 0) { s_count = 0; s_cnt1 = 0; }

  const int64_t jw = (int64_t)blockIdx.x * kThreads * 4;          // first column of the workgroup
  const int64_t j0 = jw + threadIdx.x * 4;
  const int64_t rbeg = row0 + (int64_t)blockIdx.y * kIouRowsPerWg;
  const int nrows = (int)min((int64_t)kIouRowsPerWg, row1 - rbeg);
  if (threadIdx.x < nrows) s_rows[threadIdx.x] = P1[rbeg + threadIdx.x];
  float bx[4], by[4], br[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    PreBox b = {};
    if (j0 + k < m) b = P2[j0 + k];
    bx[k] = b.x; by[k] = b.y; br[k] = b.r;
  }
  const bool vec_ok = (j0 + 3 < m) && ((m & 3) == 0);   // 16-byte aligned full group
  __syncthreads();

  // Second stage, dense: every lane takes one circle-test survivor from the LDS queue and runs the
  // separating-axis test on it (a wave with ANY surviving lane used to run the SAT for all its lanes: 86 % of
  // the iterations at a 3 % survival rate).  Column boxes come from global memory here (L2-resident, ~3 % of the
  // pairs).  Called by all threads, after a barrier that made the first-stage pushes visible.
  auto drain_q1 = [&]() {
    const unsigned cnt1 = s_cnt1;                          // stable: nobody pushes to s_q1 during a drain
    for (unsigned e0 = 0; e0 < cnt1; e0 += kThreads) {     // uniform trip count
      if (__syncthreads_or(s_count > kIouQueue - kThreads)) queue_flush(Q, gq, gcount, cap);
      const unsigned e = e0 + threadIdx.x;
      if (e < cnt1) {
        const unsigned v = s_q1[e], r = v >> 10, jl = v & 1023u;
        const PreBox B = P2[jw + jl];
        if (!sat_disjoint(s_rows[r], B)) queue_push(Q, (unsigned)(rbeg + r - row0), (unsigned)(jw + jl));
      }
    }
    __syncthreads();                                       // all entries consumed
    if (threadIdx.x == 0) s_cnt1 = 0;
    __syncthreads();
  };

  PreBox Ai = s_rows[0];
  for (int r = 0; r < nrows; r++) {
    const float ax = Ai.x, ay = Ai.y, ar = Ai.r;
    if (r + 1 < nrows) Ai = s_rows[r + 1];   // next row's box while this one is processed
    const int64_t i = rbeg + r;
    (void)i; (void)vec_ok;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (j0 + k < m && !surely_disjoint(ax, ay, ar, bx[k], by[k], br[k])) {
        const unsigned p = atomicAdd(&s_cnt1, 1u);
        s_q1[p] = (unsigned short)((r << 10) | (threadIdx.x * 4 + k));
      }
    }
    if (STORE) {
      float* dst = out + i * m + j0;
      if (vec_ok) {
        *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (j0 + k < m) dst[k] = 0.f;
      }
    }
    if ((r & 1) == 1) {          // <= 2048 pushes per two rows: the first-stage queue cannot overflow
      if (__syncthreads_or(s_cnt1 > kIouQ1DrainAt)) drain_q1();
    }
  }
  __syncthreads();
  drain_q1();
  queue_flush(Q, gq, gcount, cap);
}

// ---- pair finding beside a forked zero-fill (no stores here), with NO LDS traffic in its first stage.  A wave owns 64
// rows (lane = row) and walks its columns 64 at a time: lane j holds column j's box of the chunk in registers, v_readlane
// hands column j's circle to all lanes as scalar operands (j is a compile-time constant in the unrolled loop), the
// verdicts collect in a 64-bit mask per lane.  Second stage without a list: every lane walks its own mask bits and fetches
// the column box from the owning lane by ds_bpermute (the crossbar, not the banks); the loop runs max-popcount times
// (5-6 at DOTA-like densities).  Survivors of both tests are staged per wave, one global atomic per workgroup at the end.
// No barrier in the loop.  Circle test: (ax-bx)^2 + (ay-by)^2 > (1.002 ar + 1e-3 + 1.002 br)^2 -- surely_disjoint's
// margin with the two factors hoisted into the row and the column; NaNs compare false and are evaluated.
// (Forms that were built, tested bit-exact, measured and removed again -- DESIGN.md section 4 has the numbers: circle
// records as LDS broadcast reads with per-wave survivor lists (59 us alone became 79), the same on half the LDS, a dense
// second stage fed from a list, a grid-binned finder, and one launch per 256 x 256 tile that also fills and evaluates.)
constexpr int kCrStage = 256;                 // per-wave staged pairs
__device__ __forceinline__ float lane_bcast(float v, int j) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}
template <int J0, int J1>
__device__ __forceinline__ void circle_bits(float ax, float ay, float ar, float cx, float cy, float cr, unsigned& bits) {
  // two columns per packed-f32 instruction (v_pk_add / v_pk_mul / v_pk_fma_f32; the broadcast column pair is one scalar-pair
  // operand): 8.5 instead of 12.5 instructions per column.  The test only has to be conservative (a pair with IoU > 0 has
  // circles that overlap by the 0.2 % margin), so the fused multiply-add is fine here.
  using f2 = __attribute__((ext_vector_type(2))) float;
  const f2 ax2 = {ax, ax}, ay2 = {ay, ay}, ar2 = {ar, ar};
#pragma unroll
  for (int j = J0; j < J1; j += 2) {
    const f2 cx2 = {lane_bcast(cx, j), lane_bcast(cx, j + 1)}, cy2 = {lane_bcast(cy, j), lane_bcast(cy, j + 1)};
    const f2 cr2 = {lane_bcast(cr, j), lane_bcast(cr, j + 1)};
    const f2 dx = ax2 - cx2, dy = ay2 - cy2, R = ar2 + cr2;
    const f2 d2 = __builtin_elementwise_fma(dy, dy, dx * dx), R2 = R * R;
    bits |= (d2[0] > R2[0] ? 0u : 1u) << (j - J0);
    bits |= (d2[1] > R2[1] ? 0u : 1u) << (j + 1 - J0);
  }
}
__global__ __launch_bounds__(kThreads) void k_iou_cull_lanes(const PreBox* __restrict__ P1, const PreBox* __restrict__ P2,
                                                             int64_t row0, int64_t row1, int64_t m, int cols_per_wg,
                                                             uint2* __restrict__ gq,
                                                             unsigned long long* __restrict__ gcount,
                                                             unsigned long long cap) {
  __shared__ uint2 s_stage[kThreads / 64][kCrStage];
  __shared__ unsigned s_left[kThreads / 64];
  __shared__ unsigned long long s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wr0 = row0 + ((int64_t)blockIdx.y * (kThreads / 64) + wave) * 64;    // this wave's rows
  const int64_t row = wr0 + lane;
  const bool valid = row < row1;
  PreBox A = {};
  if (valid) A = P1[row];
  const float ax = A.x, ay = A.y, ar = A.r * 1.002f + 1e-3f;
  const int64_t jw = (int64_t)blockIdx.x * cols_per_wg;
  const int64_t jend = min(m, jw + cols_per_wg);
  uint2* stage = s_stage[wave];
  unsigned ns = 0;                               // wave-uniform
  auto flush = [&]() {
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(gcount, (unsigned long long)ns);
    base = ((unsigned long long)(uint32_t)__shfl((int)(base >> 32), 0) << 32) | (uint32_t)__shfl((int)(base & 0xffffffffu), 0);
    wave_lds_handoff();                          // other lanes' staged pairs
    for (unsigned k = lane; k < ns; k += 64)
      if (base + k < cap) gq[base + k] = stage[k];
    wave_lds_handoff();                          // ... are read before the stage is written again
    ns = 0;
  };
  PreBox Cn = {};                                // next chunk's column box of this lane (one chunk ahead)
  if (jw + lane < jend) Cn = P2[jw + lane];
  for (int64_t jc = jw; jc < jend; jc += 64) {
    const PreBox C = Cn;
    Cn = PreBox{};
    if (jc + 64 + lane < jend) Cn = P2[jc + 64 + lane];
    const int nc = (int)min((int64_t)64, jend - jc);
    // a column beyond the end gets a circle no row can reach (NaN rows reach everything: masked below)
    const float cx = C.x, cy = C.y, cr = lane < nc ? C.r * 1.002f : -3.0e38f;
    unsigned lo = 0, hi = 0;
    circle_bits<0, 32>(ax, ay, ar, cx, cy, cr, lo);
    circle_bits<32, 64>(ax, ay, ar, cx, cy, cr, hi);
    unsigned long long mask = ((unsigned long long)hi << 32) | lo;
    if (nc < 64) mask &= (1ull << nc) - 1ull;
    if (!valid) mask = 0;
    while (__any(mask != 0ull)) {
      const bool has = mask != 0ull;
      const int j = has ? __ffsll((long long)mask) - 1 : 0;
      if (has) mask &= mask - 1ull;
      PreBox B;
      B.x = __shfl(C.x, j); B.y = __shfl(C.y, j); B.w = __shfl(C.w, j); B.h = __shfl(C.h, j);
      B.c2 = __shfl(C.c2, j); B.s2 = __shfl(C.s2, j); B.r = 0.f; B.label = 0.f;
      const bool hit = has && !sat_disjoint(A, B);
      const unsigned long long bal = __ballot(hit);
      if (hit)
        stage[ns + __popcll(bal & ((1ull << lane) - 1ull))] = make_uint2((unsigned)(row - row0), (unsigned)(jc + j));
      ns += (unsigned)__popcll(bal);
      if (ns + 64 > kCrStage) flush();
    }
  }
  if (lane == 0) s_left[wave] = ns;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; w++) {
    if (w < wave) before += s_left[w];
    all += s_left[w];
  }
  if (all == 0) return;                // uniform
  if (threadIdx.x == 0) s_base = atomicAdd(gcount, (unsigned long long)all);
  __syncthreads();
  const unsigned long long base = s_base + before;
  for (unsigned k = lane; k < ns; k += 64)
    if (base + k < cap) gq[base + k] = stage[k];
}

// HEAVY: dense list, one pair per lane, persistent grid.  Values go to a compact buffer (vals[e] for pair e): this pass
// runs while the zero-fill of the output is still in flight on the side stream, so it must not touch `out`.
// Two passes: the first gives every lane 8 candidate-point slots (16 KB of LDS per workgroup instead of 48: the exact
// IoU is a chain of dependent LDS round trips and was latency-bound at 3 waves per SIMD); a pair that produces more than
// 8 candidates (shared edges, duplicates: never in general position) leaves a marker, and k_iou_scatter redoes the
// marked pairs with the full 24 slots.  A genuine result with the marker's bits would only be recomputed to itself.
__global__ __launch_bounds__(kThreads) void k_iou_heavy(const PreBox* __restrict__ P1,
                                                        const PreBox* __restrict__ P2, int64_t row0,
                                                        const uint2* __restrict__ gq,
                                                        const unsigned long long* __restrict__ gcount,
                                                        unsigned long long cap, float* __restrict__ vals) {
  __shared__ float2 s_pts[kIouCap * kThreads];
  const unsigned long long total = *gcount;
  if (total > cap) return;       // list overflow: k_iou_scatter recomputes the chunk directly
  for (unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (unsigned long long)gridDim.x * kThreads) {
    uint2 ij = gq[e];
    PreBox A = P1[row0 + ij.x];
    PreBox B = P2[ij.y];
    bool redo = false;
    const float v = rbox_iou<kThreads, kIouCap>(A, B, s_pts + threadIdx.x, &redo);
    vals[e] = redo ? __uint_as_float(kIouRedo) : v;
  }
}

// after the join with the zero-fill: out[i, j] = vals[e] for the listed pairs.  Overflow fallback: the pair list of this
// chunk did not fit (extremely dense inputs) -> recompute the whole chunk pair by pair (the divergence that the list
// avoids is irrelevant when most pairs are heavy anyway).
__global__ __launch_bounds__(kThreads) void k_iou_scatter(const PreBox* __restrict__ P1, const PreBox* __restrict__ P2,
                                                          int64_t row0, int64_t row1, int64_t m,
                                                          float* __restrict__ out, const uint2* __restrict__ gq,
                                                          const unsigned long long* __restrict__ gcount,
                                                          unsigned long long cap, const float* __restrict__ vals) {
  __shared__ float2 s_pts[24 * kThreads];
  const unsigned long long total = *gcount;
  if (total > cap) {
    const int64_t all = (row1 - row0) * m;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < all; e += (int64_t)gridDim.x * kThreads) {
      int64_t i = row0 + e / m, j = e % m;
      PreBox A = P1[i], B = P2[j];
      if (!surely_disjoint(A.x, A.y, A.r, B.x, B.y, B.r) && !sat_disjoint(A, B))
        out[i * m + j] = rbox_iou<kThreads>(A, B, s_pts + threadIdx.x);
    }
    return;
  }
  for (unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (unsigned long long)gridDim.x * kThreads) {
    const uint2 ij = gq[e];
    float v = vals[e];
    if (__float_as_uint(v) == kIouRedo)      // more than 8 candidate points in the first pass: all 24 slots here
      v = rbox_iou<kThreads>(P1[row0 + ij.x], P2[ij.y], s_pts + threadIdx.x);
    out[(row0 + ij.x) * m + ij.y] = v;
  }
}

// 16 bytes per lane, grid-stride: 7 TB/s on MI355X (profiles/r02_nms_200k_pmc_before.txt, k_zero_words)
// PACE > 0: s_sleep between the stores of a wave -- a fill that runs flat out saturates the memory system and every
// dependent read of the kernels beside it takes ~10 us (the pair finder stretched from 59 to 110 us whatever it did)
template <int PACE>
__global__ __launch_bounds__(256) void k_fill_zero(float* __restrict__ out, unsigned long long n) {
  const unsigned long long n4 = n / 4, stride = (unsigned long long)gridDim.x * 256;
  float4* o4 = reinterpret_cast<float4*>(out);
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PACE > 0) __builtin_amdgcn_s_sleep(PACE);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) out[n4 * 4 + threadIdx.x] = 0.f;
}

__global__ __launch_bounds__(kThreads) void k_iou_pairs(const float* __restrict__ b1,
                                                        const float* __restrict__ b2, int64_t n,
                                                        float* __restrict__ out) {
  __shared__ float2 s_pts[24 * kThreads];
  int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float* a = b1 + 5 * i;
  const float* b = b2 + 5 * i;
  PreBox A = make_prebox(a[0], a[1], a[2], a[3], a[4], 0.f);
  PreBox B = make_prebox(b[0], b[1], b[2], b[3], b[4], 0.f);
  out[i] = rbox_iou<kThreads>(A, B, s_pts + threadIdx.x);
}

constexpr unsigned long long kIouQueueCap = 32ull << 20;  // 32 Mi pairs = 256 MiB

}  // namespace

int build_flags_iou() { return kBuildFlags; }   // ORed into build_flags_rotated()'s bits of s2a_build_flags()
}  // namespace s2a

using namespace s2a;

// (a declared upper BOUND, not the image of a carve: the call splits whatever follows its three buffers over the two pair lists)
extern "C" size_t s2a_box_iou_rotated_workspace_bytes(int64_t n, int64_t m) {
  if (n < 0 || m < 0 || n >= (1ll << 31) || m >= (1ll << 31)) return 0;   // (sizes the entry point refuses)
  if (n == 0 || m == 0) return 256;
  unsigned long long pairs = (unsigned long long)n * (unsigned long long)m;
  unsigned long long cap = std::max<unsigned long long>(std::min<unsigned long long>(pairs, kIouQueueCap), (unsigned long long)m * 256);
  return align_up((size_t)(n + m) * sizeof(PreBox)) * 2 + align_up(cap * (sizeof(uint2) + sizeof(float))) + 8192;
}

namespace s2a {
namespace {
constexpr unsigned long long kIouForkBytes = 8ull << 20;   // smaller outputs: one stream, zero-fill fused into the cull
}  // namespace
}  // namespace s2a

extern "C" int s2a_box_iou_rotated(const float* boxes1, int64_t n, const float* boxes2, int64_t m,
                                   float* ious, void* workspace, size_t workspace_bytes,
                                   s2a_stream_t stream) {
  S2A_CHECK_ARG(n >= 0 && m >= 0, "box_iou_rotated: negative size");
  if (n == 0 || m == 0) return S2A_OK;  // reference: empty [N,M] (cuda.cu:79)
  S2A_CHECK_ARG(boxes1 && boxes2 && ious, "box_iou_rotated: NULL tensor");
  S2A_CHECK_ARG(n < (1ll << 31) && m < (1ll << 31), "box_iou_rotated: size out of range");
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_box_iou_rotated_workspace_bytes(n, m), "box_iou_rotated");
  hipStream_t st = as_stream(stream);
  Carver cv(workspace, workspace_bytes);
  PreBox* P1 = cv.take<PreBox>((size_t)n);
  PreBox* P2 = cv.take<PreBox>((size_t)m);
  unsigned long long* counters = cv.take<unsigned long long>(512);
  if (!P1 || !P2 || !counters ||
      cv.off + (size_t)m * 256 * (sizeof(uint2) + sizeof(float)) + 512 > workspace_bytes) {
    set_error("box_iou_rotated: workspace too small (%zu bytes)", workspace_bytes);
    return S2A_EWORKSPACE;
  }
  unsigned long long cap = (workspace_bytes - cv.off - 256) / (sizeof(uint2) + sizeof(float));
  uint2* gq = reinterpret_cast<uint2*>(static_cast<char*>(workspace) + cv.off);
  float* vals = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_up(cv.off + cap * sizeof(uint2)) );
  cap = std::min<unsigned long long>(cap, (workspace_bytes - (size_t)(reinterpret_cast<char*>(vals) - static_cast<char*>(workspace))) / sizeof(float));
  // rows per chunk: sized for up to 1/4 of the pairs surviving the cull (DOTA-like inputs: ~1 %);
  // a denser chunk overflows the list and is recomputed pair by pair in k_iou_scatter
  int64_t rows_per_chunk = (int64_t)std::min<unsigned long long>((unsigned long long)n, 4 * (cap / (unsigned long long)m));
  if (rows_per_chunk < n) rows_per_chunk = std::max<int64_t>(256, rows_per_chunk / 256 * 256);   // (else: one chunk)
  int64_t chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
  if (chunks > 512) {
    set_error("box_iou_rotated: workspace too small for %lld x %lld", (long long)n, (long long)m);
    return S2A_EWORKSPACE;
  }
  // Large outputs are write-bound (4 B per pair, ~1 % of DOTA-like pairs overlap): the zero-fill of the whole matrix
  // runs on a side stream at the full store rate while this stream finds the overlapping pairs and evaluates them into a
  // compact buffer; after the join a small kernel drops the values into place.  (Round 1 stored the zeros from the cull
  // kernel -- 4 TB/s beside its circle tests -- and ran the dense pass after it: 212 us at 10 k x 10 k.)
  const bool big = (unsigned long long)n * (unsigned long long)m * 4ull >= kIouForkBytes;
  const char* ef = getenv("S2A_IOU_FORK");                 // A/B: 0 = never fork, 1 = always
  const bool fork = ef && (ef[0] == '0' || ef[0] == '1') ? ef[0] == '1' : big;
  SideSet* ss = nullptr;
  hipStream_t side = nullptr;
  if (fork) {
    int rc = side_set(st, &ss);
    if (rc != S2A_OK) return rc;
    side = ss->s[0];
    S2A_HIP(hipEventRecord(ss->fork, st));
    S2A_HIP(hipStreamWaitEvent(side, ss->fork, 0));
    // The fill is PACED (s_sleep between the stores of a wave): flat out it finishes 400 MB in 50-100 us but saturates the
    // memory system, and every dependent read of the kernels beside it then takes ~10 us -- the pair finder stretched
    // from 59 to 105-125 us whatever its design and whatever the fill's workgroup count (docs/HISTORY.md, round 3).  At 512
    // workgroups and s_sleep 12 it moves ~3.5 TB/s (113 us at 10 k x 10 k), ends before the chain beside it does (pair
    // finding 62 + exact pass 60-65 us, both at their stand-alone speed) and the call takes ~157 us instead of ~195.
    int fill_wgs = 512, pace = 12;
#ifdef S2A_MEASURE
    if (const char* fw = getenv("S2A_IOU_FILL_WGS")) fill_wgs = atoi(fw);     // measurement builds only; 0 = no fill (WRONG results)
    if (const char* fp = getenv("S2A_IOU_FILL_PACE")) pace = atoi(fp);
#endif
    const unsigned long long nm = (unsigned long long)n * (unsigned long long)m;
    if (fill_wgs > 0) {
      if (pace >= 12) k_fill_zero<12><<<fill_wgs, 256, 0, side>>>(ious, nm);
      else if (pace >= 8) k_fill_zero<8><<<fill_wgs, 256, 0, side>>>(ious, nm);
      else if (pace >= 6) k_fill_zero<6><<<fill_wgs, 256, 0, side>>>(ious, nm);
      else if (pace >= 4) k_fill_zero<4><<<fill_wgs, 256, 0, side>>>(ious, nm);
      else if (pace >= 2) k_fill_zero<2><<<fill_wgs, 256, 0, side>>>(ious, nm);
      else k_fill_zero<0><<<fill_wgs, 256, 0, side>>>(ious, nm);
    }
    S2A_HIP(hipEventRecord(ss->join[0], side));
  }
  k_prep_boxes2<<<(unsigned)((std::max<int64_t>(n + m, 512) + 255) / 256), 256, 0, st>>>(boxes1, n, P1, boxes2, m, P2, counters, 512);
  const char* ec = getenv("S2A_IOU_CULL_COLS");            // A/B: round 1's column-major cull beside the forked fill
  const bool cull_cols = ec && ec[0] == '1';
  for (int64_t c = 0; c < chunks; c++) {
    int64_t r0 = c * rows_per_chunk, r1 = std::min(n, r0 + rows_per_chunk);
    dim3 grid_c((unsigned)((m + kThreads * 4 - 1) / (kThreads * 4)), (unsigned)((r1 - r0 + kIouRowsPerWg - 1) / kIouRowsPerWg));
    if (fork && !cull_cols) {
      // columns per workgroup: enough workgroups for ~8 per CU, at least 256 columns each
      const int64_t rwg = (r1 - r0 + kThreads - 1) / kThreads;
      int64_t cw = 256;
      while (cw < m && rwg * ((m + cw - 1) / cw) > 4096) cw *= 2;
      k_iou_cull_lanes<<<dim3((unsigned)((m + cw - 1) / cw), (unsigned)rwg), kThreads, 0, st>>>(P1, P2, r0, r1, m, (int)cw, gq,
                                                                                            counters + c, cap);
    }
    else if (fork)
      k_iou_cull<false><<<grid_c, kThreads, 0, st>>>(P1, P2, r0, r1, m, ious, gq, counters + c, cap);
    else
      k_iou_cull<true><<<grid_c, kThreads, 0, st>>>(P1, P2, r0, r1, m, ious, gq, counters + c, cap);
    k_iou_heavy<<<kHeavyGrid, kThreads, 0, st>>>(P1, P2, r0, gq, counters + c, cap, vals);
    if (fork && c == 0) S2A_HIP(hipStreamWaitEvent(st, ss->join[0], 0));
    k_iou_scatter<<<kPersistentGrid, kThreads, 0, st>>>(P1, P2, r0, r1, m, ious, gq, counters + c, cap, vals);
  }
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_box_iou_rotated_pairs(const float* boxes1, const float* boxes2, int64_t n,
                                         float* ious, s2a_stream_t stream) {
  S2A_CHECK_ARG(n >= 0, "box_iou_rotated_pairs: negative size");
  if (n == 0) return S2A_OK;
  S2A_CHECK_ARG(boxes1 && boxes2 && ious, "box_iou_rotated_pairs: NULL tensor");
  k_iou_pairs<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, as_stream(stream)>>>(boxes1, boxes2, n, ious);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
