// Label assignment of the training loss for MI355X (gfx950, wave64): assign_labels (models/utils.py:33-147).
// COMPILE WITH -ffp-contract=off (see rbox_geom.hpp): both ops give the same overlaps, bit for bit.
//
//   1. the BATCHED op (s2a_assign_labels_batched): every (anchor set, image) of a batch in ONE fixed launch sequence, with
//      the image sort of the targets done on the device                                      kernels k_ab_*, AbWs
//   2. the PER-IMAGE op (s2a_assign_labels), further down:
//        MATRIX form  the [M,N] overlaps from s2a_box_iou_rotated (iou_ops.hip, through the public header) and three
//                     streaming passes over them               k_assign_rows / _colmax / _colarg / _cols
//        LIST form    no matrix: cull -> pair list -> exact pass, for N <= kAtMaxN gts and M x N <= kAtMaxPairs
//                     k_assign_list_init / _cull / _exact / _rule3 / _rows_list / _last, AtWs
//        no gts       k_assign_empty
// Each op describes its workspace once: a carve() that both the call and the *_workspace_bytes query run.
// The order-preserving overlap key and the anchor validity rule that 1 and 2 must share: assign_keys.hpp.
//
// The per-image op ("LIST form") needs the host to know each image's gt count, so the head read the counts
// back and made 2*B calls of five or six launches.  In the batched op nothing depends on a device value: the launches and their
// geometry follow from the host arguments alone, there is no host read and no allocation, so the whole loss can be
// captured into a graph and replayed against new targets written into a static [G,7] table (rows with an image index
// outside [0, B) are padding).
//
//   k_ab_init          row / column accumulators, pair count, per-image histogram <- neutral values; the anchor-set table
//   k_ab_prep_count    image index of every input row (-1 = dropped) and the histogram of the images
//   k_ab_prep_offsets  exclusive scan of the histogram -> target_offsets[B+1], status[2]
//   k_ab_prep_scatter  stable counting sort: row i goes to offsets[image] + (earlier rows of the same image); PreBox of
//                      every sorted gt; the rows behind the real ones are zeroed
//   k_ab_cull          grid (anchor-row groups, B, sets): a workgroup owns 16 anchor rows of one (set, image) and walks that
//                      image's gts in LDS chunks of kAbChunk: circle + separating-axis test, survivors into an LDS list, one
//                      global reservation per chunk flush.  ONE pair list and ONE count for all problems
//   k_ab_exact         exact IoU of the listed pairs, balanced over the whole list; row maximum / first arg-max, filtered
//                      count, column maxima by atomics
//   k_ab_rule3         pairs that attain their gt's maximum: rule 3 slot of the anchor (all anchors) or the gt's first anchor
//   k_ab_last          gt_max_assign_all == 0 only: each gt's anchor takes the LAST gt that chose it (atomicMax on the rule 3
//                      slot: no per-image limit)
//   k_ab_rows          rules 1, 2, 3 and the empty-image rule per anchor; pair-list overflow -> status
//
// LDS of the cull: kAbChunk * 32 B of gts + 16 * kAbChunk * 4 B of list = 12 KiB static, whatever the gt counts are.  A CU
// holds 8 workgroups of 256 threads by its wave slots and 13 by this LDS (160 KiB), so the chunk does not limit occupancy;
// 128 gts x 16 rows are 8 ballot rounds of the 256 threads per chunk, and an image of the usual 30 gts is one short chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "assign_keys.hpp"
#include "common.hpp"
#include "rbox_geom.hpp"
#include "rotated_common.hpp"

namespace s2a {
namespace {

constexpr int kAbRows = 16;      // anchor rows per cull workgroup
constexpr int kAbChunk = 128;    // gts per LDS chunk of the cull
constexpr int kAbMaxSets = 4;

// The set table goes to the kernels through the workspace (k_ab_init writes it): a set index that is only known on the
// device would send a by-value table to scratch.  Named fields, so that k_ab_init itself indexes nothing.
struct AbSets {
  const float *a0, *a1, *a2, *a3;
  int64_t st0, st1, st2, st3;
};
struct AbSet {
  const float* anchors;
  int64_t stride;
};
__device__ __forceinline__ const float* set_anchors(const AbSet* __restrict__ tab, unsigned s, unsigned b) {
  return tab[s].anchors + (int64_t)b * tab[s].stride;
}

struct AbWs {                    // carved from the workspace, in this order
  AbSet* sets;                   // [kAbMaxSets]
  int* img;                      // [G] image of input row i, -1 = dropped
  int* img_count;                // [B]
  int* gt_img;                   // [G] image of sorted row g
  PreBox* gt_pre;                // [G] by sorted row
  int* gt_key;                   // [S*G] column maxima (keys), by sorted row
  int* gt_arg;                   // [S*G] first anchor (index within the image) attaining the maximum
  unsigned long long* rowbest;   // [S*B*A] key << 32 | ~(gt index within the image)
  int* nbad;                     // [S*B*A] filtered (negative) overlaps of the row
  int* r3;                       // [S*B*A] rule 3: last gt whose maximum the anchor attains
  unsigned long long* count;     // pairs found (may exceed the capacity)
  uint2* pair;                   // [P] (row in [S*B*A], sorted gt row)
  float* val;                    // [P]
};

bool carve(Carver& cv, int64_t S, int64_t B, int64_t A, int64_t G, int64_t P, AbWs& w) {
  const size_t g = (size_t)std::max<int64_t>(G, 1), rows = (size_t)(S * B * A), p = (size_t)std::max<int64_t>(P, 1);
  w.sets = cv.take<AbSet>(kAbMaxSets);
  w.img = cv.take<int>(g);
  w.img_count = cv.take<int>((size_t)B);
  w.gt_img = cv.take<int>(g);
  w.gt_pre = cv.take<PreBox>(g);
  w.gt_key = cv.take<int>((size_t)S * g);
  w.gt_arg = cv.take<int>((size_t)S * g);
  w.rowbest = cv.take<unsigned long long>(rows);
  w.nbad = cv.take<int>(rows);
  w.r3 = cv.take<int>(rows);
  w.count = cv.take<unsigned long long>(1);
  w.pair = cv.take<uint2>(p);
  w.val = cv.take<float>(p);
  return cv.ok();
}
constexpr size_t kAbWsSlack = 1024;   // headroom the query has always declared; no sub-buffer lives in it

__global__ __launch_bounds__(256) void k_ab_init(AbSets t, AbWs w, int64_t rows, int64_t cols, int B) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < rows) { w.rowbest[i] = 0ull; w.nbad[i] = 0; w.r3[i] = -1; }
  if (i < cols) { w.gt_key[i] = 0; w.gt_arg[i] = 0x7fffffff; }
  if (i < B) w.img_count[i] = 0;
  if (i == 0) {
    *w.count = 0ull;
    w.sets[0] = AbSet{t.a0, t.st0};
    w.sets[1] = AbSet{t.a1, t.st1};
    w.sets[2] = AbSet{t.a2, t.st2};
    w.sets[3] = AbSet{t.a3, t.st3};
  }
}

__global__ __launch_bounds__(256) void k_ab_prep_count(const float* __restrict__ targets, int64_t G,
                                                       const int64_t* __restrict__ num_targets, int B, AbWs w) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= G) return;
  int64_t n = num_targets ? *num_targets : G;
  n = n < 0 ? 0 : n > G ? G : n;
  int b = -1;
  if (i < n) {
    const float f = targets[7 * i];
    if (f > -1.f && f < (float)B) b = (int)f;                    // (int64)f in [0, B): truncation, as .long()
  }
  w.img[i] = b;
  if (b >= 0) atomicAdd(w.img_count + b, 1);
}

// one wave: exclusive scan of the image histogram
__global__ __launch_bounds__(64) void k_ab_prep_offsets(int B, AbWs w, int64_t* __restrict__ offsets,
                                                        int64_t* __restrict__ status) {
  const int lane = threadIdx.x;
  int64_t run = 0;
  for (int base = 0; base < B; base += 64) {
    const int i = base + lane;
    const int c = i < B ? w.img_count[i] : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (i < B) offsets[i] = run + (int64_t)(incl - c);
    run += (int64_t)__shfl(incl, 63);
  }
  if (lane == 0) {
    offsets[B] = run;
    status[0] = 0;                                               // bit 0 comes from k_ab_rows; bit 1 is never needed here
    status[2] = run;
    status[3] = 0;
  }
}

// Stable: the rank of row i is the number of EARLIER rows of its image (G^2 / 2 LDS compares in all: 29 k at the 240 rows
// of a B = 8 batch, 8 M at 4 096 rows)
__global__ __launch_bounds__(256) void k_ab_prep_scatter(const float* __restrict__ targets, int64_t G, int B, AbWs w,
                                                         const int64_t* __restrict__ offsets,
                                                         float* __restrict__ sorted) {
  __shared__ int s_img[256];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const int mine = i < G ? w.img[i] : -1;
  int rank = 0;
  for (int64_t t0 = 0; t0 <= (int64_t)blockIdx.x * 256; t0 += 256) {
    s_img[tid] = t0 + tid < G ? w.img[t0 + tid] : -1;
    __syncthreads();
    const int lim = i - t0 < 256 ? (int)(i - t0) : 256;         // the own tile: the rows in front of i only
    if (mine >= 0)
      for (int k = 0; k < lim; k++) rank += s_img[k] == mine ? 1 : 0;
    __syncthreads();
  }
  if (i >= G) return;
  if (mine >= 0) {
    const int64_t pos = offsets[mine] + rank;
    const float* t = targets + 7 * i;
    float* o = sorted + 7 * pos;
#pragma unroll
    for (int k = 0; k < 7; k++) o[k] = t[k];
    w.gt_pre[pos] = make_prebox(t[2], t[3], t[4], t[5], t[6], 0.f);
    w.gt_img[pos] = mine;
  }
  if (i >= offsets[B]) {                                          // behind the real rows: zero
    float* o = sorted + 7 * i;
#pragma unroll
    for (int k = 0; k < 7; k++) o[k] = 0.f;
    PreBox z = {};
    w.gt_pre[i] = z;
    w.gt_img[i] = 0;
  }
}

__global__ __launch_bounds__(256) void k_ab_cull(int64_t A, const int64_t* __restrict__ offsets, float img_h,
                                                 float img_w, int filt_anchor, unsigned long long cap, AbWs w) {
  __shared__ PreBox s_gt[kAbChunk];
  __shared__ uint32_t s_list[kAbRows * kAbChunk];
  __shared__ PreBox s_anc[kAbRows];
  __shared__ uint8_t s_valid[kAbRows];
  __shared__ unsigned s_cnt;
  __shared__ unsigned long long s_base;
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned b = blockIdx.y, s = blockIdx.z;
  const int64_t g0 = offsets[b];
  const int N = (int)(offsets[b + 1] - g0);
  if (N == 0) return;                                             // (uniform) the empty-image rule is k_ab_rows'
  const int64_t m0 = (int64_t)blockIdx.x * kAbRows;
  const float* anchors = set_anchors(w.sets, s, b);
  if (tid < kAbRows) {
    const int64_t m = m0 + tid;
    bool valid = false;
    PreBox P = {};
    if (m < A) {
      const float* a = anchors + 5 * m;
      valid = !filt_anchor || anchor_valid(a, img_h, img_w);      // invalid anchors: every overlap is -0.5 (:97-98), nothing to list
      P = make_prebox(a[0], a[1], a[2], a[3], a[4], 0.f);
    }
    s_anc[tid] = P;
    s_valid[tid] = valid ? 1 : 0;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  bool any = false;
#pragma unroll
  for (int r = 0; r < kAbRows; r++) any |= s_valid[r] != 0;
  if (!any) return;                                               // (uniform) e.g. a whole level of oversized anchors
  const unsigned row0 = (unsigned)(((int64_t)s * gridDim.y + b) * A + m0);
  for (int c0 = 0; c0 < N; c0 += kAbChunk) {
    const int cn = min(kAbChunk, N - c0);
    for (int j = tid; j < cn; j += 256) s_gt[j] = w.gt_pre[g0 + c0 + j];
    __syncthreads();
    const int total = kAbRows * cn;
    for (int i0 = 0; i0 < total; i0 += 256) {
      const int idx = i0 + tid;
      bool hit = false;
      int r = 0, j = 0;
      if (idx < total) {
        r = idx / cn; j = idx - r * cn;
        if (s_valid[r]) {
          const PreBox& P = s_anc[r];
          const PreBox& Q = s_gt[j];
          hit = !surely_disjoint(P.x, P.y, P.r, Q.x, Q.y, Q.r) && !sat_disjoint(P, Q);
        }
      }
      const unsigned long long bal = __ballot(hit);
      if (bal) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(&s_cnt, (unsigned)__popcll(bal));
        base = (unsigned)__shfl((int)base, 0);
        if (hit) s_list[base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = ((uint32_t)r << 16) | (uint32_t)j;
      }
    }
    __syncthreads();
    const unsigned cnt = s_cnt;                                   // <= kAbRows * kAbChunk: the LDS list cannot overflow
    if (cnt != 0) {                                               // (uniform)
      if (tid == 0) s_base = atomicAdd(w.count, (unsigned long long)cnt);   // always counted ...
      __syncthreads();
      const unsigned long long base = s_base;
      for (unsigned e = tid; e < cnt; e += 256) {
        const uint32_t rj = s_list[e];
        if (base + e < cap)                                       // ... written below the capacity only
          w.pair[base + e] = make_uint2(row0 + (rj >> 16), (unsigned)(g0 + c0) + (rj & 0xffffu));
      }
    }
    __syncthreads();
    if (tid == 0) s_cnt = 0;                                      // seen after the next chunk's barrier
  }
}

__global__ __launch_bounds__(256) void k_ab_exact(unsigned A, unsigned B, int64_t G,
                                                  const int64_t* __restrict__ offsets, int filt_iou,
                                                  unsigned long long cap, AbWs w) {
  __shared__ float2 s_pts[24 * 256];
  const unsigned long long total = min(*w.count, cap);
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
    const uint2 mj = w.pair[e];
    const unsigned sb = mj.x / A, m = mj.x - sb * A, s = sb / B, b = sb - s * B;
    const float* a = set_anchors(w.sets, s, b) + 5 * (int64_t)m;
    const PreBox P = make_prebox(a[0], a[1], a[2], a[3], a[4], 0.f);
    float v = rbox_iou<256>(P, w.gt_pre[mj.y], s_pts + threadIdx.x);
    if (filt_iou && !(v >= 0.f && v <= 1.f)) v = -0.5f;          // :86-93
    v += 0.f;                                                    // -0.0 -> +0.0
    w.val[e] = v;
    if (v < 0.f) atomicAdd(w.nbad + mj.x, 1);
    else if (v > 0.f) {
      const int k = iou_key(v);
      const uint32_t j = (uint32_t)((int64_t)mj.y - offsets[b]); // the gt's index within its image
      atomicMax(w.rowbest + mj.x, ((unsigned long long)(uint32_t)k << 32) | (unsigned long long)(0xffffffffu - j));
      atomicMax(w.gt_key + (int64_t)s * G + mj.y, k);
    }
  }
}

__global__ __launch_bounds__(256) void k_ab_rule3(unsigned A, unsigned B, int64_t G, const int64_t* __restrict__ offsets,
                                                  float min_pos_thr, int assign_all, unsigned long long cap, AbWs w) {
  const unsigned long long total = min(*w.count, cap);
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
    const float v = w.val[e];
    if (!(v > 0.f)) continue;
    const uint2 mj = w.pair[e];
    const unsigned sb = mj.x / A, m = mj.x - sb * A, s = sb / B, b = sb - s * B;
    const int kc = w.gt_key[(int64_t)s * G + mj.y];
    if (key_iou(kc) > min_pos_thr && iou_key(v) == kc) {         // :126: this anchor attains the gt's maximum
      if (assign_all) atomicMax(w.r3 + mj.x, (int)((int64_t)mj.y - offsets[b]));
      else atomicMin(w.gt_arg + (int64_t)s * G + mj.y, (int)m);
    }
  }
}

// one anchor per gt (gt_max_assign_all = False): gt j's anchor is the first row attaining its maximum (gt_arg); the
// reference's ascending loop lets a later gt overwrite an earlier one on the same anchor: the largest j wins the slot
__global__ __launch_bounds__(256) void k_ab_last(int64_t A, int B, int64_t G, int64_t cols,
                                                 const int64_t* __restrict__ offsets, float min_pos_thr, AbWs w) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cols) return;
  const int mine = w.gt_arg[t];
  if (!(key_iou(w.gt_key[t]) > min_pos_thr) || mine == 0x7fffffff) return;   // (rows behind the real ones: key 0)
  const int64_t s = t / G, g = t - s * G;
  const int b = w.gt_img[g];
  atomicMax(w.r3 + (s * B + b) * A + mine, (int)(g - offsets[b]));
}

__global__ __launch_bounds__(256) void k_ab_rows(unsigned A, unsigned B, int64_t rows,
                                                 const int64_t* __restrict__ offsets, float img_h, float img_w,
                                                 float pos_thr, float neg_thr, int filt_anchor, unsigned long long cap,
                                                 AbWs w, int64_t* __restrict__ assign, int64_t* __restrict__ status) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  if (row == 0) {
    const unsigned long long c = *w.count;
    status[1] = (int64_t)c;
    if (c > cap) status[0] |= 1;                                  // (k_ab_prep_offsets wrote status[0] earlier in the stream)
  }
  const unsigned sb = (unsigned)(row / A), m = (unsigned)(row - (int64_t)sb * A), s = sb / B, b = sb - s * B;
  const bool valid = !filt_anchor || anchor_valid(set_anchors(w.sets, s, b) + 5 * (int64_t)m, img_h, img_w);
  const int64_t N = offsets[b + 1] - offsets[b];
  int64_t a = -2;
  if (N == 0) {
    a = valid ? -1 : -2;                                          // :72-80 no gt boxes: valid anchors are negatives
  } else {
    const unsigned long long best_k = w.rowbest[row];
    float best = 0.f;                                             // every entry that was not listed is an exact zero
    int64_t arg = 0;
    if (!valid || (int64_t)w.nbad[row] == N) best = -0.5f;        // :97-98 / every overlap filtered
    else if (best_k != 0ull) { best = key_iou((int)(best_k >> 32)); arg = (int64_t)(0xffffffffu - (uint32_t)(best_k & 0xffffffffull)); }
    if (best >= 0.f && best < neg_thr) a = -1;                    // :108
    if (best >= pos_thr) a = arg;                                 // :114-115
    const int r3 = w.r3[row];
    if (r3 >= 0) a = r3;                                          // :131-145: the last gt that takes this anchor
  }
  assign[row] = a;
}

// ================================================================= the per-image op (s2a_assign_labels), MATRIX form
// assign_labels (models/utils.py:33-147): the real consumer of box_iou_rotated in the reference.  The [M,N]
// matrix comes from the cull -> pair list -> dense pass pipeline of iou_ops.hip (a per-anchor loop over the gts was 10x
// slower: divergence); three streaming passes over it replace the reference's dozen tensor ops and its
// Python loop over the gts: (1) one wave per anchor row: validity / range filters in place, row max and
// first arg-max, rules 1 and 2(1); (2) column maxima (tiled, atomicMax on order-preserving keys);
// (3) one wave per row: the LAST gt whose column maximum the anchor attains (the reference's ascending loop
// lets later gts overwrite earlier ones, :131-145).
// iou_key / key_iou / anchor_valid: assign_keys.hpp (shared with the batched form above)
__global__ __launch_bounds__(256) void k_assign_rows(const float* __restrict__ anchors, float* __restrict__ ious,
                                                     int64_t M, int64_t N, float img_h, float img_w, float pos_thr,
                                                     float neg_thr, int filt_anchor, int filt_iou,
                                                     int64_t* __restrict__ assign) {
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const bool valid = !filt_anchor || anchor_valid(anchors + 5 * m, img_h, img_w);
  float* row = ious + m * N;
  float best = -2.f;
  int64_t arg = 0;
  for (int64_t j = lane; j < N; j += 64) {
    float v = row[j];
    if (filt_iou && !(v >= 0.f && v <= 1.f)) v = -0.5f;        // :86-93
    if (!valid) v = -0.5f;                                     // :97-98
    v += 0.f;                                                  // -0.0 -> +0.0
    row[j] = v;
    if (v > best) { best = v; arg = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int64_t oa = __shfl_xor(arg, o);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }   // first index of the maximum
  }
  if (lane == 0) {
    int64_t a = -2;
    if (best >= 0.f && best < neg_thr) a = -1;                 // :108
    if (best >= pos_thr) a = arg;                              // :114-115
    assign[m] = a;
  }
}

// grid (ceil(N/64), ceil(M/256)): thread = one column over 256 rows; rows are read 64 columns wide (coalesced)
__global__ __launch_bounds__(64) void k_assign_colmax(const float* __restrict__ ious, int64_t M, int64_t N,
                                                      int* __restrict__ gt_key) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= N) return;
  const int64_t m0 = (int64_t)blockIdx.y * 256, m1 = min(M, m0 + 256);
  int k = 0;
  for (int64_t m = m0; m < m1; m++) k = max(k, iou_key(ious[m * N + j]));
  if (k > 0) atomicMax(gt_key + j, k);
}

__global__ __launch_bounds__(64) void k_assign_colarg(const float* __restrict__ ious, int64_t M, int64_t N,
                                                      const int* __restrict__ gt_key, int* __restrict__ gt_arg) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= N) return;
  const int64_t m0 = (int64_t)blockIdx.y * 256, m1 = min(M, m0 + 256);
  const int k = gt_key[j];
  for (int64_t m = m0; m < m1; m++)
    if (iou_key(ious[m * N + j]) == k) { atomicMin(gt_arg + j, (int)m); break; }   // first row of this chunk
}

__global__ __launch_bounds__(256) void k_assign_cols(const float* __restrict__ ious, int64_t M, int64_t N,
                                                     float min_pos_thr, const int* __restrict__ gt_key,
                                                     const int* __restrict__ gt_arg, int64_t* __restrict__ assign) {
  const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= M) return;
  const float* row = ious + m * N;
  int64_t best = -1;
  for (int64_t j = lane; j < N; j += 64) {
    const int k = gt_key[j];
    if (!(key_iou(k) > min_pos_thr)) continue;                 // :126
    const bool hit = gt_arg ? gt_arg[j] == (int)m : iou_key(row[j]) == k;
    if (hit) best = j;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  if (lane == 0 && best >= 0) assign[m] = best;
}

// ---- LIST form (round 6): no [M,N] matrix.  The matrix form above is eleven launches (the IoU pipeline alone five) and a
// strided column-maximum pass: 146 us at 32 gts, 211 us at 300 -- slower than the unfused pair at the sizes models/utils.py:33
// sees.  Here, for N <= kAtMaxN gts and M x N pairs that fit the list:
//   k_assign_cull   a workgroup owns 16 anchor rows with ALL gts in LDS: circle + separating-axis test of its 16 x N pairs,
//                   the survivors into an LDS list, ONE global reservation per workgroup, (row, gt) pairs out;
//   k_assign_exact  exact IoU of the listed pairs, every lane busy and the whole chip balanced (the 64 P7 anchors of a chip
//                   overlap most gts: owned by one workgroup they took 0.5 ms): value kept in the list; row maximum / first
//                   arg-max, the count of filtered entries and the column maxima by atomics;
//   k_assign_rule3  with the final column maxima: the pairs that attain one -> rule 3 (all anchors), or the first such row;
//   k_assign_rows   rules 1, 2 (and 3) per anchor; k_assign_last when one anchor per gt is taken.
// Exact zeros never enter the list (a disjoint pair is 0.0 by the reference's own num == 0 return), so the row rules start
// from "all zero" and only count filtered (negative) entries.  Needs min_pos_iou_thr >= 0 and pos_iou_thr > 0.
constexpr int kAtRows = 16, kAtMaxN = 1024;
constexpr unsigned long long kAtMaxPairs = 8ull << 20;       // list capacity = M x N (never overflows), at most this
struct AtWs {                                                // carved from the workspace, in this order
  PreBox* gt_pre; int* gt_key; int* gt_arg; unsigned long long* rowbest; int* nbad; int* r3; unsigned long long* count;
  uint2* pair; float* val;
};
// the one description of the list form's buffers: s2a_assign_labels carves them, the workspace query sums them
bool carve(Carver& cv, int64_t M, int64_t N, AtWs& w) {
  const size_t mn = (size_t)M * (size_t)N;
  w.gt_pre = cv.take<PreBox>((size_t)N);
  w.gt_key = cv.take<int>((size_t)N);
  w.gt_arg = cv.take<int>((size_t)N);
  w.rowbest = cv.take<unsigned long long>((size_t)M);
  w.nbad = cv.take<int>((size_t)M);
  w.r3 = cv.take<int>((size_t)M);
  w.count = cv.take<unsigned long long>(1);
  w.pair = cv.take<uint2>(mn);
  w.val = cv.take<float>(mn);
  return cv.ok();
}
// the matrix form's: the [M,N] IoU matrix, the column maxima / arg-maxima, and s2a_box_iou_rotated's own workspace
struct AmWs { float* ious; int *gt_key, *gt_arg; char* iou_ws; size_t iou_bytes; };
bool carve(Carver& cv, int64_t M, int64_t N, AmWs& w) {
  w.ious = cv.take<float>((size_t)M * N);
  w.gt_key = cv.take<int>((size_t)N);
  w.gt_arg = cv.take<int>((size_t)N);
  w.iou_bytes = s2a_box_iou_rotated_workspace_bytes(M, N);
  w.iou_ws = cv.take<char>(w.iou_bytes);
  return cv.ok();
}
constexpr size_t kAssignWsSlack = 1024;   // headroom the query has always declared over either form; no sub-buffer lives in it
__global__ void k_assign_list_init(const float* __restrict__ gt, int N, int64_t M, AtWs w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    const float* g = gt + 5 * i;
    w.gt_pre[i] = make_prebox(g[0], g[1], g[2], g[3], g[4], 0.f);
    w.gt_key[i] = 0;
    w.gt_arg[i] = 0x7fffffff;
  }
  if (i < M) { w.rowbest[i] = 0ull; w.nbad[i] = 0; w.r3[i] = -1; }
  if (i == 0) *w.count = 0ull;
}

__global__ __launch_bounds__(256) void k_assign_cull(const float* __restrict__ anchors, int64_t M, int N, float img_h, float img_w,
                                                     int filt_anchor, AtWs w) {
  extern __shared__ __attribute__((aligned(16))) char smem_at[];
  PreBox* s_gt = reinterpret_cast<PreBox*>(smem_at);                                       // [N]
  uint32_t* s_list = reinterpret_cast<uint32_t*>(smem_at + (size_t)N * sizeof(PreBox));    // [kAtRows * N]
  __shared__ PreBox s_anc[kAtRows];
  __shared__ uint8_t s_valid[kAtRows];
  __shared__ unsigned s_cnt;
  __shared__ unsigned long long s_base;
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t m0 = (int64_t)blockIdx.x * kAtRows;
  for (int j = tid; j < N; j += 256) s_gt[j] = w.gt_pre[j];
  if (tid < kAtRows) {
    const int64_t m = m0 + tid;
    bool valid = false;
    PreBox A = {};
    if (m < M) {
      const float* a = anchors + 5 * m;
      valid = !filt_anchor || anchor_valid(a, img_h, img_w);     // invalid anchors: every overlap is -0.5 (:97-98), nothing to list
      A = make_prebox(a[0], a[1], a[2], a[3], a[4], 0.f);
    }
    s_anc[tid] = A;
    s_valid[tid] = valid ? 1 : 0;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  const int total = kAtRows * N;
  for (int i0 = 0; i0 < total; i0 += 256) {
    const int idx = i0 + tid;
    bool hit = false;
    int r = 0, j = 0;
    if (idx < total) {
      r = idx / N; j = idx - r * N;
      if (s_valid[r]) {
        const PreBox& A = s_anc[r];
        const PreBox& B = s_gt[j];
        hit = !surely_disjoint(A.x, A.y, A.r, B.x, B.y, B.r) && !sat_disjoint(A, B);
      }
    }
    const unsigned long long bal = __ballot(hit);
    if (bal) {
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(&s_cnt, (unsigned)__popcll(bal));
      base = (unsigned)__shfl((int)base, 0);
      if (hit) s_list[base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = ((uint32_t)r << 16) | (uint32_t)j;
    }
  }
  __syncthreads();
  const unsigned cnt = s_cnt;
  if (cnt == 0) return;                                          // (uniform)
  if (tid == 0) s_base = atomicAdd(w.count, (unsigned long long)cnt);
  __syncthreads();
  const unsigned long long base = s_base;
  for (unsigned e = tid; e < cnt; e += 256) {
    const uint32_t rj = s_list[e];
    w.pair[base + e] = make_uint2((unsigned)(m0 + (rj >> 16)), rj & 0xffffu);
  }
}

__global__ __launch_bounds__(256) void k_assign_exact(const float* __restrict__ anchors, int filt_iou, AtWs w) {
  __shared__ float2 s_pts[24 * 256];
  const unsigned long long total = *w.count;
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
    const uint2 mj = w.pair[e];
    const float* a = anchors + 5 * (int64_t)mj.x;
    const PreBox A = make_prebox(a[0], a[1], a[2], a[3], a[4], 0.f);
    float v = rbox_iou<256>(A, w.gt_pre[mj.y], s_pts + threadIdx.x);
    if (filt_iou && !(v >= 0.f && v <= 1.f)) v = -0.5f;          // :86-93
    v += 0.f;                                                    // -0.0 -> +0.0
    w.val[e] = v;
    if (v < 0.f) atomicAdd(w.nbad + mj.x, 1);
    else if (v > 0.f) {
      const int k = iou_key(v);
      atomicMax(w.rowbest + mj.x, ((unsigned long long)(uint32_t)k << 32) | (unsigned long long)(0xffffffffu - mj.y));
      atomicMax(w.gt_key + mj.y, k);
    }
  }
}

__global__ __launch_bounds__(256) void k_assign_rule3(float min_pos_thr, int assign_all, AtWs w) {
  const unsigned long long total = *w.count;
  for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
    const float v = w.val[e];
    if (!(v > 0.f)) continue;
    const uint2 mj = w.pair[e];
    const int kc = w.gt_key[mj.y];
    if (key_iou(kc) > min_pos_thr && iou_key(v) == kc) {         // :126: this anchor attains the gt's maximum
      if (assign_all) atomicMax(w.r3 + mj.x, (int)mj.y);
      else atomicMin(w.gt_arg + mj.y, (int)mj.x);
    }
  }
}

__global__ void k_assign_rows_list(const float* __restrict__ anchors, int64_t M, int N, float img_h, float img_w, float pos_thr,
                                   float neg_thr, int filt_anchor, int assign_all, AtWs w, int64_t* __restrict__ assign) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  const bool valid = !filt_anchor || anchor_valid(anchors + 5 * m, img_h, img_w);
  const unsigned long long b = w.rowbest[m];
  float best = 0.f;                                              // every entry that was not listed is an exact zero
  int64_t arg = 0;
  if (!valid || w.nbad[m] == N) best = -0.5f;                    // :97-98 / every overlap filtered
  else if (b != 0ull) { best = key_iou((int)(b >> 32)); arg = (int64_t)(0xffffffffu - (uint32_t)(b & 0xffffffffull)); }
  int64_t a = -2;
  if (best >= 0.f && best < neg_thr) a = -1;                     // :108
  if (best >= pos_thr) a = arg;                                  // :114-115
  if (assign_all && w.r3[m] >= 0) a = w.r3[m];                   // :131-145: the last gt whose maximum the anchor attains
  assign[m] = a;
}

// one anchor per gt (gt_max_assign_all = False): gt j's anchor is the first row attaining its maximum (gt_arg); the
// reference's ascending loop lets a later gt overwrite an earlier one on the same anchor
__global__ __launch_bounds__(1024) void k_assign_last(const int* __restrict__ gt_key, const int* __restrict__ gt_arg, int N,
                                                      float min_pos_thr, int64_t* __restrict__ assign) {
  __shared__ int s_m[kAtMaxN];
  const int j = threadIdx.x;
  int mine = -1;
  if (j < N && key_iou(gt_key[j]) > min_pos_thr && gt_arg[j] != 0x7fffffff) mine = gt_arg[j];
  if (j < kAtMaxN) s_m[j] = mine;
  __syncthreads();
  if (mine < 0) return;
  for (int k = j + 1; k < N; k++)
    if (s_m[k] == mine) return;
  assign[mine] = j;
}

// no gt boxes (:72-80): valid anchors are negatives, the others stay ignored
__global__ void k_assign_empty(const float* __restrict__ anchors, int64_t M, float img_h, float img_w, int filt_anchor,
                               int64_t* __restrict__ assign) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  assign[m] = (!filt_anchor || anchor_valid(anchors + 5 * m, img_h, img_w)) ? -1 : -2;
}

}  // namespace

int build_flags_assign() { return kBuildFlags; }   // ORed into build_flags_rotated()'s bits of s2a_build_flags()
}  // namespace s2a

using namespace s2a;

extern "C" size_t s2a_assign_labels_batched_workspace_bytes(int64_t num_sets, int64_t batch, int64_t num_anchors,
                                                            int64_t target_capacity, int64_t pair_capacity) {
  if (num_sets < 1 || num_sets > kAbMaxSets || batch < 1 || num_anchors < 1 || target_capacity < 0 || pair_capacity < 0 ||
      batch > 65535 || num_sets * batch * num_anchors >= (1ll << 32) || num_sets * target_capacity >= (1ll << 31) ||
      pair_capacity >= (1ll << 40))
    return 0;
  return carved_bytes<AbWs>(num_sets, batch, num_anchors, target_capacity, pair_capacity) + kAbWsSlack;
}

extern "C" int s2a_assign_labels_batched(const s2a_anchor_set* sets, int num_sets, int64_t batch, int64_t num_anchors,
                                         const float* targets, int64_t target_capacity, const int64_t* num_targets,
                                         float img_h, float img_w, float pos_iou_thr, float neg_iou_thr,
                                         float min_pos_iou_thr, int gt_max_assign_all, int filter_invalid_anchors,
                                         int filter_invalid_ious, int64_t* assign_ids, float* sorted_targets,
                                         int64_t* target_offsets, int64_t* status, int64_t pair_capacity, void* workspace,
                                         size_t workspace_bytes, s2a_stream_t stream) {
  const int64_t S = num_sets, B = batch, A = num_anchors, G = target_capacity, P = pair_capacity;
  S2A_CHECK_ARG(S >= 1 && S <= kAbMaxSets, "assign_labels_batched: 1 to %d anchor sets, got %d", kAbMaxSets, num_sets);
  S2A_CHECK_ARG(B >= 1 && A >= 1 && G >= 0 && P >= 0, "assign_labels_batched: negative or empty size (batch %lld, anchors %lld, "
                "target_capacity %lld, pair_capacity %lld)", (long long)B, (long long)A, (long long)G, (long long)P);
  S2A_CHECK_ARG(B <= 65535 && S * B * A < (1ll << 32) && S * G < (1ll << 31) && P < (1ll << 40),
                "assign_labels_batched: sizes out of range (batch <= 65535, sets x batch x anchors < 2^32, sets x targets < 2^31)");
  S2A_CHECK_ARG(sets && assign_ids && target_offsets && status && ((targets && sorted_targets) || G == 0),
                "assign_labels_batched: NULL tensor");
  const float* set_ptr[kAbMaxSets] = {};
  int64_t set_stride[kAbMaxSets] = {};
  for (int s = 0; s < num_sets; s++) {
    S2A_CHECK_ARG(sets[s].anchors, "assign_labels_batched: NULL tensor (anchors of set %d)", s);
    S2A_CHECK_ARG(sets[s].batch_stride == 0 || sets[s].batch_stride >= A * 5,
                  "assign_labels_batched: batch_stride of set %d must be 0 (shared) or >= 5 x anchors", s);
    set_ptr[s] = sets[s].anchors;
    set_stride[s] = sets[s].batch_stride;
  }
  const AbSets t = {set_ptr[0], set_ptr[1], set_ptr[2], set_ptr[3], set_stride[0], set_stride[1], set_stride[2], set_stride[3]};
  S2A_CHECK_ARG(min_pos_iou_thr >= 0.f && pos_iou_thr > 0.f,
                "assign_labels_batched: needs min_pos_iou_thr >= 0 and pos_iou_thr > 0 (unlisted pairs count as exact zeros)");
  AbWs w;
  if (int rc = carve_workspace(workspace, workspace_bytes, w, kAbWsSlack, "assign_labels_batched", S, B, A, G, P)) return rc;
  S2A_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "assign_labels_batched: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int64_t rows = S * B * A, cols = S * G;
  const unsigned long long cap = (unsigned long long)P;
  const auto blocks = [](int64_t n) { return (unsigned)((std::max<int64_t>(n, 1) + 255) / 256); };
  k_ab_init<<<blocks(std::max(rows, std::max(cols, B))), 256, 0, st>>>(t, w, rows, cols, (int)B);
  if (G > 0) k_ab_prep_count<<<blocks(G), 256, 0, st>>>(targets, G, num_targets, (int)B, w);
  k_ab_prep_offsets<<<1, 64, 0, st>>>((int)B, w, target_offsets, status);
  if (G > 0) {
    k_ab_prep_scatter<<<blocks(G), 256, 0, st>>>(targets, G, (int)B, w, target_offsets, sorted_targets);
    k_ab_cull<<<dim3((unsigned)((A + kAbRows - 1) / kAbRows), (unsigned)B, (unsigned)S), 256, 0, st>>>(
        A, target_offsets, img_h, img_w, filter_invalid_anchors, cap, w);
    k_ab_exact<<<1024, 256, 0, st>>>((unsigned)A, (unsigned)B, G, target_offsets, filter_invalid_ious, cap, w);
    k_ab_rule3<<<1024, 256, 0, st>>>((unsigned)A, (unsigned)B, G, target_offsets, min_pos_iou_thr, gt_max_assign_all, cap, w);
    if (!gt_max_assign_all) k_ab_last<<<blocks(cols), 256, 0, st>>>(A, (int)B, G, cols, target_offsets, min_pos_iou_thr, w);
  }
  k_ab_rows<<<blocks(rows), 256, 0, st>>>((unsigned)A, (unsigned)B, rows, target_offsets, img_h, img_w, pos_iou_thr,
                                          neg_iou_thr, filter_invalid_anchors, cap, w, assign_ids, status);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" size_t s2a_assign_labels_workspace_bytes(int64_t num_anchors, int64_t num_gts) {
  if (num_anchors < 0 || num_gts < 0 || num_anchors >= (1ll << 31) || num_gts >= (1ll << 31)) return 0;   // (refused sizes)
  const int64_t M = std::max<int64_t>(num_anchors, 1), N = std::max<int64_t>(num_gts, 1);
  const size_t matrix_form = carved_bytes<AmWs>(M, N);
  const size_t list_form = (unsigned long long)M * (unsigned long long)N <= kAtMaxPairs ? carved_bytes<AtWs>(M, N) : 0;
  return std::max(matrix_form, list_form) + kAssignWsSlack;
}

extern "C" int s2a_assign_labels(const float* anchors, int64_t num_anchors, const float* gt_boxes, int64_t num_gts,
                                 float img_h, float img_w, float pos_iou_thr, float neg_iou_thr, float min_pos_iou_thr,
                                 int gt_max_assign_all, int filter_invalid_anchors, int filter_invalid_ious,
                                 int64_t* assign_gt_ids, void* workspace, size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(num_anchors >= 0 && num_gts >= 0 && num_anchors < (1ll << 31) && num_gts < (1ll << 31),
                "assign_labels: sizes out of range");
  if (num_anchors == 0) return S2A_OK;
  S2A_CHECK_ARG(anchors && assign_gt_ids && (gt_boxes || num_gts == 0), "assign_labels: NULL tensor");
  hipStream_t st = as_stream(stream);
  const int64_t M = num_anchors, N = num_gts;
  if (N == 0) {
    k_assign_empty<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(anchors, M, img_h, img_w, filter_invalid_anchors, assign_gt_ids);
    S2A_LAUNCH_CHECK();
    return S2A_OK;
  }
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_assign_labels_workspace_bytes(M, N), "assign_labels");
  // list form: no IoU matrix, five short launches (see k_assign_cull).  S2A_ASSIGN_LIST=0: the matrix form (A/B, tests)
  {
    const char* e = std::getenv("S2A_ASSIGN_LIST");
    const unsigned long long mn = (unsigned long long)M * (unsigned long long)N;
    if (N <= kAtMaxN && mn <= kAtMaxPairs && min_pos_iou_thr >= 0.f && pos_iou_thr > 0.f && !(e && e[0] == '0')) {
      AtWs w;
      if (int rc = carve_workspace(workspace, workspace_bytes, w, kAssignWsSlack, "assign_labels", M, N)) return rc;
      const size_t lds = (size_t)N * sizeof(PreBox) + (size_t)kAtRows * N * 4;
      static bool attr_set = false;
      if (!attr_set) {
        S2A_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_assign_cull), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(kAtMaxN * sizeof(PreBox) + (size_t)kAtRows * kAtMaxN * 4)));
        attr_set = true;
      }
      const int64_t mx = std::max<int64_t>(M, N);
      k_assign_list_init<<<(unsigned)((mx + 255) / 256), 256, 0, st>>>(gt_boxes, (int)N, M, w);
      k_assign_cull<<<(unsigned)((M + kAtRows - 1) / kAtRows), 256, lds, st>>>(anchors, M, (int)N, img_h, img_w, filter_invalid_anchors, w);
      k_assign_exact<<<1024, 256, 0, st>>>(anchors, filter_invalid_ious, w);
      k_assign_rule3<<<1024, 256, 0, st>>>(min_pos_iou_thr, gt_max_assign_all, w);
      k_assign_rows_list<<<(unsigned)((M + 255) / 256), 256, 0, st>>>(anchors, M, (int)N, img_h, img_w, pos_iou_thr, neg_iou_thr,
                                                                      filter_invalid_anchors, gt_max_assign_all, w, assign_gt_ids);
      if (!gt_max_assign_all)
        k_assign_last<<<1, 1024, 0, st>>>(w.gt_key, w.gt_arg, (int)N, min_pos_iou_thr, assign_gt_ids);
      S2A_LAUNCH_CHECK();
      return S2A_OK;
    }
  }
  AmWs w;
  if (int rc = carve_workspace(workspace, workspace_bytes, w, kAssignWsSlack, "assign_labels", M, N)) return rc;
  int rc = s2a_box_iou_rotated(anchors, M, gt_boxes, N, w.ious, w.iou_ws, w.iou_bytes, stream);
  if (rc != S2A_OK) return rc;
  fill_u32(w.gt_key, 0u, (size_t)N, st);
  const unsigned gr = (unsigned)((M + 3) / 4);
  k_assign_rows<<<gr, 256, 0, st>>>(anchors, w.ious, M, N, img_h, img_w, pos_iou_thr, neg_iou_thr, filter_invalid_anchors,
                                    filter_invalid_ious, assign_gt_ids);
  dim3 gc((unsigned)((N + 63) / 64), (unsigned)((M + 255) / 256));
  k_assign_colmax<<<gc, 64, 0, st>>>(w.ious, M, N, w.gt_key);
  if (!gt_max_assign_all) {
    fill_u32(w.gt_arg, 0x7f7f7f7fu, (size_t)N, st);
    k_assign_colarg<<<gc, 64, 0, st>>>(w.ious, M, N, w.gt_key, w.gt_arg);
  }
  k_assign_cols<<<gr, 256, 0, st>>>(w.ious, M, N, min_pos_iou_thr, w.gt_key, gt_max_assign_all ? nullptr : w.gt_arg, assign_gt_ids);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
