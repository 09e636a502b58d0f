// Whole-scene detection on the device: the chip gather in front of the detector and the per-class polygon merge behind it.
//
// The reference does both offline: DOTA_devkit/SplitOnlyImage_multi_process.py:39-85 writes 1024 x 1024 chips (zero padded,
// saveimagepatches :39-49) to disk, val.py:40-52 writes one text line per detection, and
// DOTA_devkit/ResultMerge_multi_process.py:178-245 parses the lines, moves every polygon back into scene coordinates
// (poly2origpoly :178-185) and runs py_cpu_nms_poly_fast (:62-123) once per (scene, class).  Here:
//   s2a_scene_gather_u8  one launch copies every chip of a batch out of the HWC uint8 scene;
//   s2a_scene_merge      takes the detector's padded per-chip output as it is and returns the merged detections of the
//                        scene, class-major and by descending score -- no host synchronisation, no device-to-host copy,
//                        no memset node (legal under stream capture), no n x n / 64 mask.
// The merge is ONE greedy resolve over the whole list: rows are sorted by (class, score descending, row index), suppression
// edges are only ever formed inside a class segment, so the resolve by rounds that the polygon NMS uses (rotated_ops.hip)
// settles every class at once.  COMPILE WITH -ffp-contract=off (polyiou and the coordinate shift are compared bit for bit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "poly_geom.hpp"

namespace s2a {
namespace {

// ---------------------------------------------------------------- chip gather
// A chip row is subsize * 3 bytes; its source starts at ((up + y) * W + left) * 3: byte aligned only.  One thread owns 16
// destination bytes (one aligned 16-byte store).  Inside the scene it reads the five aligned dwords that hold its 16 source
// bytes and shifts them into place (neighbouring lanes share a dword: the second read hits the cache, HBM sees every byte
// once); a chunk that touches the scene's border, or whose aligned reads would pass the end of the buffer, goes byte by
// byte with the zero padding of saveimagepatches (:45-46).
__global__ __launch_bounds__(256) void k_scene_gather(const uint8_t* __restrict__ scene, int64_t H, int64_t W,
                                                      const int32_t* __restrict__ origins, int64_t total_chunks,
                                                      int32_t subsize, uint8_t* __restrict__ chips) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total_chunks) return;
  const int32_t row_bytes = subsize * 3, row_chunks = row_bytes / 16;
  const int32_t ch = (int32_t)(t % row_chunks);
  const int64_t ry = t / row_chunks;
  const int32_t y = (int32_t)(ry % subsize);
  const int64_t chip = ry / subsize;
  const int64_t left = origins[2 * chip], up = origins[2 * chip + 1];
  const int64_t sy = up + y, b0 = left * 3 + (int64_t)ch * 16;      // source row, first source byte inside that row
  const int64_t scene_bytes = H * W * 3;
  uint4 out = make_uint4(0u, 0u, 0u, 0u);
  if (sy >= 0 && sy < H) {
    const int64_t a = sy * W * 3 + b0, a0 = a & ~(int64_t)3;
    if (b0 >= 0 && b0 + 16 <= W * 3 && a0 + 20 <= scene_bytes) {
      const uint32_t* s = reinterpret_cast<const uint32_t*>(scene + a0);
      const uint32_t d0 = s[0], d1 = s[1], d2 = s[2], d3 = s[3], d4 = s[4];
      const uint32_t sh = (uint32_t)(a & 3) * 8;
      out.x = (uint32_t)((((unsigned long long)d1 << 32) | d0) >> sh);
      out.y = (uint32_t)((((unsigned long long)d2 << 32) | d1) >> sh);
      out.z = (uint32_t)((((unsigned long long)d3 << 32) | d2) >> sh);
      out.w = (uint32_t)((((unsigned long long)d4 << 32) | d3) >> sh);
    } else {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (int k = 0; k < 16; k++) {
        const int64_t b = b0 + k;
        if (b >= 0 && b < W * 3) w[k >> 2] |= (uint32_t)scene[sy * W * 3 + b] << (8 * (k & 3));
      }
      out = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  *reinterpret_cast<uint4*>(chips + (chip * subsize + y) * (int64_t)row_bytes + (int64_t)ch * 16) = out;
}

// ---------------------------------------------------------------- scene merge
struct MergeCtl {
  unsigned long long pairs;     // HBB-overlapping pairs inside a class (true total, may exceed the list)
  unsigned long long edges;     // pairs whose polygon IoU suppresses
};

__device__ __forceinline__ uint32_t f32_sortable(float f) {
  if (f == 0.0f) f = 0.0f;                                    // -0 == +0 in numpy's compare
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// key = class << 32 | ~score: an ascending STABLE radix sort lists the rows class-major, by descending score, ties by
// ascending row index (chip-major, then detection order) -- the order py_cpu_nms_poly_fast's argsort of s2a_nms_poly gives.
// Rows behind a chip's count, or without a class (-1 padding), get class == num_classes: they sort behind every real row.
__global__ void k_scene_keys(const float* __restrict__ dets, const int32_t* __restrict__ labels,
                             const int32_t* __restrict__ counts, int64_t n, int32_t K, int32_t num_classes,
                             unsigned long long* __restrict__ key, int32_t* __restrict__ idx, MergeCtl* __restrict__ ctl,
                             long long* __restrict__ class_counts) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r == 0) *ctl = MergeCtl{0ull, 0ull};
  if (r < num_classes) class_counts[r] = 0;
  if (r >= n) return;
  const int64_t chip = r / K;
  const int32_t k = (int32_t)(r - chip * K), lb = labels[r];
  const bool valid = k < counts[chip] && lb >= 0 && lb < num_classes;
  key[r] = valid ? ((unsigned long long)(uint32_t)lb << 32) | (uint32_t)~f32_sortable(dets[6 * r + 5])
                 : ((unsigned long long)(uint32_t)num_classes << 32) | 0xffffffffull;
  idx[r] = (int32_t)r;
}

// sorted rows: the float32 polygon of s2a_rbox_to_poly widened to double, then (coordinate + chip origin) / rate in double
// (poly2origpoly :178-185: add, then divide); the axis-aligned box as py_cpu_nms_poly_fast takes it (:64-67).  Also the
// segment table: seg_start[c] = first position of class c, seg_start[num_classes] = number of real rows.
__global__ void k_scene_prep(const unsigned long long* __restrict__ key_s, const int32_t* __restrict__ order,
                             const float* __restrict__ polys32, const int32_t* __restrict__ origins,
                             const double* __restrict__ rates, int64_t n, int32_t K, int32_t num_classes,
                             PolyBox* __restrict__ sorted, uint32_t* __restrict__ seg_start) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t c = (int32_t)(key_s[p] >> 32);
  const int32_t cprev = p ? (int32_t)(key_s[p - 1] >> 32) : -1;
  for (int32_t cc = cprev + 1; cc <= c; cc++) seg_start[cc] = (uint32_t)p;
  if (p == n - 1)
    for (int32_t cc = c + 1; cc <= num_classes + 1; cc++) seg_start[cc] = (uint32_t)n;
  if (c >= num_classes) return;
  const int64_t r = order[p], chip = r / K;
  const double ox = (double)origins[2 * chip], oy = (double)origins[2 * chip + 1];
  const double rate = rates ? rates[chip] : 1.0;
  const float* q = polys32 + 8 * r;
  PolyBox b;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    b.c[2 * k] = ((double)q[2 * k] + ox) / rate;
    b.c[2 * k + 1] = ((double)q[2 * k + 1] + oy) / rate;
  }
  b.x1 = fmin(fmin(b.c[0], b.c[2]), fmin(b.c[4], b.c[6]));
  b.y1 = fmin(fmin(b.c[1], b.c[3]), fmin(b.c[5], b.c[7]));
  b.x2 = fmax(fmax(b.c[0], b.c[2]), fmax(b.c[4], b.c[6]));
  b.y2 = fmax(fmax(b.c[1], b.c[3]), fmax(b.c[5], b.c[7]));
  sorted[p] = b;
}

// Candidate pairs: k_poly_cull's shape (256 rows x 1 024 columns per workgroup, the boxes' bounds as outward-rounded floats
// in LDS, the exact double test hbb_inter > 0 of :87-93 on the float survivors, ONE reservation in the pair list per
// workgroup) restricted to the class segments: a row only looks at columns behind it AND in front of its segment's end, and
// a workgroup whose rows and columns share no class leaves at once.  Every pair py_cpu_nms_poly_fast would hand to iou_poly
// is listed (no IoU bound here: ctl->pairs is that script's own count, which is what an overflow report has to state).
constexpr int kSceneCols = 1024;
__global__ __launch_bounds__(256) void k_scene_cull(const PolyBox* __restrict__ sorted,
                                                    const unsigned long long* __restrict__ key_s,
                                                    const uint32_t* __restrict__ seg_start, int32_t num_classes,
                                                    uint2* __restrict__ pairs, MergeCtl* __restrict__ ctl,
                                                    unsigned long long cap) {
  const int64_t n = seg_start[num_classes];      // real rows
  const int64_t r0 = (int64_t)blockIdx.y * 256, c0 = (int64_t)blockIdx.x * kSceneCols;
  if (r0 >= n || c0 >= n) return;
  if (c0 + kSceneCols - 1 <= r0) return;         // every column of the chunk is at or in front of every row: no j > i
  const int64_t row_last = min(r0 + 255, n - 1);
  if (c0 > row_last && (key_s[c0] >> 32) != (key_s[row_last] >> 32)) return;   // (sorted: the first column's class is the smallest)
  __shared__ float4 s_hbb[kSceneCols];           // x1 (down), y1 (down), x2 (up), y2 (up)
  for (int k = threadIdx.x; k < kSceneCols; k += 256) {
    const float qn = __builtin_nanf("");
    float4 v = make_float4(qn, qn, qn, qn);      // (beyond the last row: every comparison below is false)
    if (c0 + k < n) {
      const PolyBox& b = sorted[c0 + k];
      v = make_float4(__double2float_rd(b.x1), __double2float_rd(b.y1), __double2float_ru(b.x2), __double2float_ru(b.y2));
    }
    s_hbb[k] = v;
  }
  __syncthreads();
  const int64_t i = r0 + threadIdx.x;
  float fx1 = __builtin_nanf(""), fy1 = fx1, fx2 = fx1, fy2 = fx1;
  int64_t seg_end = 0;
  if (i < n) {
    const PolyBox& a = sorted[i];
    fx1 = __double2float_rd(a.x1); fy1 = __double2float_rd(a.y1); fx2 = __double2float_ru(a.x2); fy2 = __double2float_ru(a.y2);
    seg_end = seg_start[(uint32_t)(key_s[i] >> 32) + 1];
  }
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_row0 = r0 + (threadIdx.x & ~63);
  unsigned long long masks[kSceneCols / 64];
  unsigned cnt = 0;
#pragma unroll
  for (int cb = 0; cb < kSceneCols / 64; cb++) {
    const int64_t j0 = c0 + cb * 64;
    unsigned long long mine = 0;
    if (j0 < n && j0 + 63 > wave_row0) {         // (wave-uniform: inside the list, not wholly in front of this wave's rows)
#pragma unroll 8
      for (int c = 0; c < 64; c++) {
        const float4 hb = s_hbb[cb * 64 + c];
        // w * h > 0 in double needs min(x2) > max(x1) and min(y2) > max(y1): the outward-rounded floats keep every such pair
        if (fx2 > hb.x && hb.z > fx1 && fy2 > hb.y && hb.w > fy1 && j0 + c > i && j0 + c < seg_end) mine |= 1ull << c;
      }
      if (mine) {                                // the exact test of the few float survivors
        const PolyBox& A = sorted[i];
        unsigned long long keep = 0;
        for (unsigned long long m = mine; m; m &= m - 1) {
          const int c = __ffsll((long long)m) - 1;
          const PolyBox& B = sorted[j0 + c];
          const double w = fmax(0.0, fmin(A.x2, B.x2) - fmax(A.x1, B.x1));
          const double h = fmax(0.0, fmin(A.y2, B.y2) - fmax(A.y1, B.y1));
          if (w * h > 0) keep |= 1ull << c;
        }
        mine = keep;
      }
    }
    masks[cb] = mine;
    cnt += (unsigned)__popcll(mine);
  }
  unsigned incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)incl, o);
    if (lane >= (unsigned)o) incl += t;
  }
  __shared__ unsigned s_wtot[4];
  __shared__ unsigned long long s_base;
  if (lane == 63) s_wtot[wave] = incl;
  __syncthreads();
  const unsigned total = s_wtot[0] + s_wtot[1] + s_wtot[2] + s_wtot[3];
  if (total == 0) return;                        // (uniform)
  if (threadIdx.x == 0) s_base = atomicAdd(&ctl->pairs, (unsigned long long)total);
  __syncthreads();
  unsigned before = incl - cnt;
  for (unsigned w2 = 0; w2 < wave; w2++) before += s_wtot[w2];
  unsigned long long slot = s_base + before;
#pragma unroll
  for (int cb = 0; cb < kSceneCols / 64; cb++) {
    unsigned long long mine = masks[cb];
    const int64_t j0 = c0 + cb * 64;
    while (mine) {
      const int c = __ffsll((long long)mine) - 1;
      mine &= mine - 1;
      if (slot < cap) pairs[slot] = make_uint2((unsigned)i, (unsigned)(j0 + c));
      slot++;
    }
  }
}

// ---- compaction of the kept rows, in the sorted order (= class-major, descending score): kept rows per block of 1 024
// positions, then prefix of the block counts + in-block scan + the output rows; positions at and behind the kept total are
// cleared, so the whole of every output buffer is defined.
constexpr int kOutRows = 1024;
__device__ __forceinline__ unsigned block_sum256(unsigned v, unsigned* s4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor((int)v, o);
  __syncthreads();                               // (s4 may still be read from the previous use)
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return s4[0] + s4[1] + s4[2] + s4[3];
}

__global__ __launch_bounds__(256) void k_scene_count(const uint8_t* __restrict__ keep_orig, const int32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ seg_start, int32_t num_classes,
                                                     uint32_t* __restrict__ cnt) {
  __shared__ unsigned s4[4];
  const int64_t n = seg_start[num_classes];
  const int64_t p0 = (int64_t)blockIdx.x * kOutRows, p1 = min(n, p0 + kOutRows);
  unsigned c = 0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) c += keep_orig[order[p]] ? 1u : 0u;
  c = block_sum256(c, s4);
  if (threadIdx.x == 0) cnt[blockIdx.x] = c;
}

__global__ __launch_bounds__(256) void k_scene_write(const uint8_t* __restrict__ keep_orig, const int32_t* __restrict__ order,
                                                     const unsigned long long* __restrict__ key_s,
                                                     const uint32_t* __restrict__ seg_start, int32_t num_classes,
                                                     const uint32_t* __restrict__ cnt, int nb, int64_t n_rows,
                                                     const PolyBox* __restrict__ sorted, const float* __restrict__ dets,
                                                     const MergeCtl* __restrict__ ctl, unsigned long long cap,
                                                     double* __restrict__ out_polys, double* __restrict__ out_scores,
                                                     long long* __restrict__ out_labels, long long* __restrict__ out_src,
                                                     long long* __restrict__ class_counts, long long* __restrict__ status) {
  __shared__ unsigned s4[4];
  __shared__ unsigned s_w[4];
  const int64_t n = seg_start[num_classes];
  unsigned mine_before = 0, mine_all = 0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const unsigned v = cnt[b];
    mine_all += v;
    if (b < (int)blockIdx.x) mine_before += v;
  }
  const unsigned before = block_sum256(mine_before, s4);
  const unsigned total = block_sum256(mine_all, s4);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[0] = ctl->pairs > cap ? 1 : 0;
    status[1] = (long long)ctl->pairs;
    status[2] = (long long)ctl->edges;
    status[3] = (long long)n;
  }
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = (int64_t)blockIdx.x * kOutRows, p1 = min(n_rows, p0 + kOutRows);
  unsigned running = before;
  for (int64_t base = p0; base < p1; base += 256) {
    const int64_t p = base + threadIdx.x;
    int64_t row = 0;
    bool f = false;
    if (p < n) { row = order[p]; f = keep_orig[row] != 0; }
    const unsigned long long bal = __ballot(f);
    __syncthreads();
    if (lane == 0) s_w[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned off = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
    for (unsigned w2 = 0; w2 < wave; w2++) off += s_w[w2];
    const int32_t c = f ? (int32_t)(key_s[p] >> 32) : -1;
    if (f) {
      const int64_t slot = (int64_t)running + off;
      const PolyBox& b = sorted[p];
#pragma unroll
      for (int k = 0; k < 8; k++) out_polys[8 * slot + k] = b.c[k];
      out_scores[slot] = (double)dets[6 * row + 5];
      out_labels[slot] = c;
      out_src[slot] = row;
    }
    // kept rows per class: positions are sorted by class, so a wave nearly always holds one class -- one atomic for the
    // lanes that share the first kept lane's class, one each for the rest
    if (bal) {
      const int32_t c_first = __shfl(c, __ffsll((long long)bal) - 1);
      const unsigned long long same = __ballot(f && c == c_first);
      if (lane == (unsigned)(__ffsll((long long)bal) - 1))
        atomicAdd(reinterpret_cast<unsigned long long*>(class_counts + c_first), (unsigned long long)__popcll(same));
      if (f && c != c_first) atomicAdd(reinterpret_cast<unsigned long long*>(class_counts + c), 1ull);
    }
    running += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (p < p1 && p >= (int64_t)total) {
#pragma unroll
      for (int k = 0; k < 8; k++) out_polys[8 * p + k] = 0.0;
      out_scores[p] = 0.0;
      out_labels[p] = -1;
      out_src[p] = -1;
    }
  }
}

__global__ void k_scene_empty(int32_t num_classes, long long* __restrict__ class_counts, long long* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < num_classes) class_counts[i] = 0;
  if (i < 4) status[i] = 0;
}

size_t scene_pair_cap(int64_t n, int64_t pair_capacity) {
  if (pair_capacity > 0) return (size_t)pair_capacity;
  const size_t all = (size_t)n * (size_t)(n > 0 ? n - 1 : 0) / 2;        // (the default of the polygon NMS's pair list)
  return std::min(all, std::max<size_t>((size_t)n * 32, (size_t)1 << 20)) + 1;
}
constexpr int kMaxClasses = 1024;
size_t scene_sort_scratch(size_t n) { return n * 40 + (8u << 20); }
struct MergeWs {                          // carved from the workspace, in this order
  unsigned long long *key_a, *key_s; int32_t *idx_a, *order; float* polys32; PolyBox* sorted; uint8_t* keep_orig;   // [n] ([n * 8])
  MergeCtl* ctl; uint32_t *seg_start, *cnt;            // 1, [kMaxClasses + 2], [n / kOutRows, rounded up]
  void* rp; uint2 *pairs, *edges, *alive;              // rocPRIM sort scratch of rpb bytes; [cap] each
  void* rounds_ws;                                     // launch_nms_edge_rounds' own, rounds_bytes
  size_t rpb, cap, rounds_bytes;
};
bool carve(Carver& cv, int64_t n, int64_t pair_capacity, MergeWs& w) {
  const size_t sz = (size_t)n;
  w.key_a = cv.take<unsigned long long>(sz);
  w.key_s = cv.take<unsigned long long>(sz);
  w.idx_a = cv.take<int32_t>(sz);
  w.order = cv.take<int32_t>(sz);
  w.polys32 = cv.take<float>(sz * 8);
  w.sorted = cv.take<PolyBox>(sz);
  w.keep_orig = cv.take<uint8_t>(sz);
  w.ctl = cv.take<MergeCtl>(1);
  w.seg_start = cv.take<uint32_t>(kMaxClasses + 2);
  w.cnt = cv.take<uint32_t>((sz + kOutRows - 1) / kOutRows);
  w.rpb = scene_sort_scratch(sz);
  w.rp = cv.take<char>(w.rpb);
  w.cap = scene_pair_cap(n, pair_capacity);
  w.pairs = cv.take<uint2>(w.cap);
  w.edges = cv.take<uint2>(w.cap);
  w.alive = cv.take<uint2>(w.cap);
  w.rounds_bytes = nms_edge_rounds_workspace(n);
  w.rounds_ws = cv.take<char>(w.rounds_bytes);
  return cv.ok();
}
constexpr size_t kMergeWsSlack = 4096;   // headroom the query has always declared; no sub-buffer lives in it

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" int s2a_scene_gather_u8(const uint8_t* scene, int64_t height, int64_t width, const int32_t* origins,
                                   int64_t n_chips, int32_t subsize, uint8_t* chips, s2a_stream_t stream) {
  S2A_CHECK_ARG(height >= 0 && width >= 0 && n_chips >= 0, "scene_gather_u8: negative size");
  S2A_CHECK_ARG(subsize > 0 && subsize % 16 == 0 && subsize <= 32768, "scene_gather_u8: subsize must be a multiple of 16 (16-byte chip rows)");
  S2A_CHECK_ARG(height * width < (1ll << 40), "scene_gather_u8: scene too large");
  if (n_chips == 0) return S2A_OK;
  S2A_CHECK_ARG(chips && origins && (scene || height * width == 0), "scene_gather_u8: NULL tensor");
  S2A_CHECK_ARG(((uintptr_t)chips % 16) == 0 && ((uintptr_t)scene % 4) == 0, "scene_gather_u8: chips must be 16-byte aligned, scene 4-byte aligned");
  const int64_t total = n_chips * subsize * (int64_t)(subsize * 3 / 16);
  S2A_CHECK_ARG((total + 255) / 256 < (1ll << 31), "scene_gather_u8: too many chips for one launch");
  k_scene_gather<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(scene, height, width, origins, total, subsize, chips);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" size_t s2a_scene_merge_workspace_bytes(int64_t n_rows, int64_t pair_capacity) {
  if (n_rows < 0 || n_rows >= (1ll << 31)) return 0;   // (sizes the entry point refuses)
  if (n_rows == 0) return 256;
  return carved_bytes<MergeWs>(n_rows, pair_capacity) + kMergeWsSlack;
}

extern "C" int s2a_scene_merge(const float* dets, const int32_t* labels, const int32_t* counts, const int32_t* origins,
                               const double* rates, int64_t n_chips, int64_t K, int32_t num_classes, double thresh,
                               int64_t pair_capacity, double* out_polys, double* out_scores, int64_t* out_labels,
                               int64_t* out_src, int64_t* class_counts, int64_t* status, void* workspace,
                               size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(n_chips >= 0 && K >= 0 && K < (1ll << 31), "scene_merge: negative size");
  S2A_CHECK_ARG(num_classes >= 1 && num_classes <= kMaxClasses, "scene_merge: num_classes must be in [1, 1024]");
  S2A_CHECK_ARG(class_counts && status, "scene_merge: class_counts / status must not be NULL");
  S2A_CHECK_ARG(n_chips == 0 || K == 0 || n_chips < (1ll << 31) / K, "scene_merge: more than 2^31 rows is not supported");
  const int64_t n = n_chips * K;
  hipStream_t st = as_stream(stream);
  if (n == 0) {
    k_scene_empty<<<(num_classes + 255) / 256, 256, 0, st>>>(num_classes, reinterpret_cast<long long*>(class_counts),
                                                             reinterpret_cast<long long*>(status));
    S2A_LAUNCH_CHECK();
    return S2A_OK;
  }
  S2A_CHECK_ARG(dets && labels && counts && origins && out_polys && out_scores && out_labels && out_src, "scene_merge: NULL tensor");
  MergeWs w;
  if (int rc = carve_workspace(workspace, workspace_bytes, w, kMergeWsSlack, "scene_merge", n, pair_capacity)) return rc;
  const size_t sz = (size_t)n, cap = w.cap;
  const int nb = (int)((sz + kOutRows - 1) / kOutRows);
  const unsigned g = (unsigned)((std::max<int64_t>(n, num_classes) + 255) / 256);
  k_scene_keys<<<g, 256, 0, st>>>(dets, labels, counts, n, (int32_t)K, num_classes, w.key_a, w.idx_a, w.ctl,
                                  reinterpret_cast<long long*>(class_counts));
  size_t need = 0;
  S2A_HIP(rocprim::radix_sort_pairs(nullptr, need, w.key_a, w.key_s, w.idx_a, w.order, sz, 0, 48, st));
  if (need > w.rpb) {
    set_error("scene_merge: workspace too small (sort scratch %zu < %zu bytes)", w.rpb, need);
    return S2A_EWORKSPACE;
  }
  S2A_HIP(rocprim::radix_sort_pairs(w.rp, need, w.key_a, w.key_s, w.idx_a, w.order, sz, 0, 48, st));
  int rc = s2a_rbox_to_poly(dets, n, 6, w.polys32, stream);
  if (rc != S2A_OK) return rc;
  k_scene_prep<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(w.key_s, w.order, w.polys32, origins, rates, n, (int32_t)K, num_classes, w.sorted,
                                                            w.seg_start);
  k_scene_cull<<<dim3((unsigned)((n + kSceneCols - 1) / kSceneCols), (unsigned)((n + 255) / 256)), 256, 0, st>>>(
      w.sorted, w.key_s, w.seg_start, num_classes, w.pairs, w.ctl, (unsigned long long)cap);
  const unsigned hb = (unsigned)std::min<size_t>((cap + kPolyThreads - 1) / kPolyThreads, 256 * 16);
  k_poly_edges<<<hb, kPolyThreads, 0, st>>>(w.sorted, w.pairs, &w.ctl->pairs, (unsigned long long)cap, thresh, w.edges, &w.ctl->edges);
  S2A_LAUNCH_CHECK();
  rc = launch_nms_edge_rounds(w.edges, (unsigned long long)cap, &w.ctl->edges, w.alive, (unsigned long long)cap, n, w.order, w.keep_orig,
                              w.rounds_ws, w.rounds_bytes, st);
  if (rc != S2A_OK) return rc;
  k_scene_count<<<nb, 256, 0, st>>>(w.keep_orig, w.order, w.seg_start, num_classes, w.cnt);
  k_scene_write<<<nb, 256, 0, st>>>(w.keep_orig, w.order, w.key_s, w.seg_start, num_classes, w.cnt, nb, n, w.sorted, dets, w.ctl,
                                    (unsigned long long)cap, out_polys, out_scores, reinterpret_cast<long long*>(out_labels),
                                    reinterpret_cast<long long*>(out_src), reinterpret_cast<long long*>(class_counts),
                                    reinterpret_cast<long long*>(status));
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
