// DOTA Task-1 evaluation of ALL classes on the device: detections + ground truth in, per-class AP / P / R / F1 out.
//
// The reference scores one class per call (voc_eval, DOTA_devkit/dota_evaluation_task1.py:92-318) and val.py:332-399 loops
// over the classes, then takes the max-F1 point of every curve.  s2a_eval_task1 does the whole of that in ONE fixed launch
// sequence -- no host synchronisation, no device-to-host copy, no memset node (legal under stream capture):
//   k_eval_det_keys / k_eval_class_keys / k_eval_group_keys + three stable radix sorts
//                      rank order = class-major, descending score, ties by ascending input row (:183 per class); a second
//                      order of the same rows by (class, image) for the overlap search
//   k_eval_gt_keys + one stable radix sort, k_eval_tables
//                      ground truth grouped by (class, image), input order kept inside a group; group offsets and the class
//                      segment table by binary search (no counters to clear)
//   k_eval_match       :204-263: first-maximum iou_poly(GT, det) over the detection's (class, image) group behind the +1-pixel
//                      axis-aligned prefilter (:223-252), bit-equal to k_poly_match; one integer atomicMin of the rank on the
//                      claimed ground truth
//   k_eval_mark / k_eval_tile_scan / k_eval_cum
//                      :265-290 as a parallel rule: of the detections that qualify for a ground truth the smallest rank is the
//                      TP, the others are FP (the best ground truth of a detection does not depend on what is taken already);
//                      integer inclusive scans of tp and fp over the whole rank order, a class's curve is a difference
//   k_eval_class       one workgroup per class: npos, rec / prec (:301-309), suffix maximum of prec, AP by the 11-point rule
//                      (:62-70) or the area rule (:72-88), the max-F1 point of val.py:357-386
//   k_eval_finish      the per-class outputs, and the optional curves with the rows behind the last real detection cleared
// Integer atomics only; every floating-point sum runs in a fixed order: two runs give the same bits.
// COMPILE WITH -ffp-contract=off (polyiou and the curve arithmetic are compared bit for bit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "poly_geom.hpp"

namespace s2a {
namespace {

constexpr int kEvalChunk = 64;         // k_eval_match: ground truths of a group staged in LDS at a time (one mask word)
constexpr int kEvalScanTile = 1024;    // k_eval_mark / k_eval_cum: rank positions per workgroup
constexpr int kEvalPerThread = 4;
constexpr int kEvalClassTile = 1024 * kEvalPerThread;   // k_eval_class: positions of a class segment per step
constexpr int kEvalMaxClasses = 1024;
constexpr uint32_t kNoGroup = 0xffffffffu;   // a key no group has

struct EvalT11 {
  double t[11];
};

__device__ __forceinline__ bool row_real(int32_t label, int32_t image, int32_t C, int32_t I) {
  return label >= 0 && label < C && image >= 0 && image < I;
}

// ---------------------------------------------------------------- keys
// ~sortable(score): an ascending stable sort lists descending scores, equal scores by ascending row (-0 == +0 as numpy
// compares them).  A padding row's score is never read.
__global__ void k_eval_det_keys(const double* __restrict__ scores, const int32_t* __restrict__ labels,
                                const int32_t* __restrict__ image, int64_t D, int32_t C, int32_t I,
                                unsigned long long* __restrict__ key, int32_t* __restrict__ idx) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= D) return;
  unsigned long long k = ~0ull;
  if (row_real(labels[r], image[r], C, I)) {
    double s = scores[r];
    if (s == 0.0) s = 0.0;
    k = ~dbl_sortable(s);
  }
  key[r] = k;
  idx[r] = (int32_t)r;
}

// second pass key: the class of the row at score position p (padding: C, behind every class)
__global__ void k_eval_class_keys(const int32_t* __restrict__ ord1, const int32_t* __restrict__ labels,
                                  const int32_t* __restrict__ image, int64_t D, int32_t C, int32_t I,
                                  uint32_t* __restrict__ ckey) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= D) return;
  const int32_t r = ord1[p];
  const int32_t lb = labels[r];
  ckey[p] = row_real(lb, image[r], C, I) ? (uint32_t)lb : (uint32_t)C;
}

// third pass: rank p -> (class, image) group; a stable sort keeps the ranks of a group ascending
__global__ void k_eval_group_keys(const uint32_t* __restrict__ ckey_s, const int32_t* __restrict__ order,
                                  const int32_t* __restrict__ image, int64_t D, int32_t C, int32_t I,
                                  uint32_t* __restrict__ gkey, int32_t* __restrict__ rank) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= D) return;
  const uint32_t c = ckey_s[p];
  gkey[p] = c < (uint32_t)C ? c * (uint32_t)I + (uint32_t)image[order[p]] : (uint32_t)C * (uint32_t)I;
  rank[p] = (int32_t)p;
}

__global__ void k_eval_gt_keys(const int32_t* __restrict__ labels, const int32_t* __restrict__ image, int64_t G, int32_t C,
                               int32_t I, uint32_t* __restrict__ key, int32_t* __restrict__ idx) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const int32_t lb = labels[g], im = image[g];
  key[g] = row_real(lb, im, C, I) ? (uint32_t)lb * (uint32_t)I + (uint32_t)im : (uint32_t)C * (uint32_t)I;
  idx[g] = (int32_t)g;
}

__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, int64_t n, uint32_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return (uint32_t)lo;
}

// gt_off[k] = first sorted ground truth of group k (k = class * I + image; gt_off[C * I] = real ground truths),
// seg_start[c] = first rank of class c (seg_start[C] = real detections), claim[slot] = "nobody yet"
__global__ void k_eval_tables(const uint32_t* __restrict__ gtkey_s, int64_t G, const uint32_t* __restrict__ ckey_s, int64_t D,
                              int32_t C, int32_t I, uint32_t* __restrict__ gt_off, uint32_t* __restrict__ seg_start,
                              int32_t* __restrict__ claim) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t groups = (int64_t)C * I;
  if (t <= groups) gt_off[t] = lower_bound_u32(gtkey_s, G, (uint32_t)t);
  if (t <= C) seg_start[t] = lower_bound_u32(ckey_s, D, (uint32_t)t);
  if (t < G) claim[t] = 0x7fffffff;
}

// ---------------------------------------------------------------- match + claim
// 128 consecutive rows of the (class, image) order per workgroup.  Ground truths are sorted by the same key, so the lists of
// all groups the workgroup's rows belong to are ONE contiguous range of the sorted ground truths: it comes through LDS in
// chunks of 64 (polygon + axis-aligned box) that every row shares, and every row looks at the part of a chunk that is its
// own group: the prefilter of :223-246 into a mask word, then iou_poly on the survivors only, in ascending order
// (np.argmax: first maximum).  Rows of different groups work side by side (a class with few rows per image has many groups
// per workgroup); a chunk that no row needs (groups without detections in between) is skipped.  Results go to the row's
// RANK position.
__global__ __launch_bounds__(kPolyThreads) void k_eval_match(
    const uint32_t* __restrict__ gkey_s, const int32_t* __restrict__ grp_rank, const int32_t* __restrict__ order, int64_t D,
    const double* __restrict__ det_polys, const double* __restrict__ gt_polys, const int32_t* __restrict__ gt_order,
    const uint8_t* __restrict__ gt_difficult, const uint32_t* __restrict__ gt_off, uint32_t groups, double ovthresh,
    int filter_difficult, double* __restrict__ ov_ws, int32_t* __restrict__ slot_ws, int32_t* __restrict__ claim) {
  __shared__ D2 s_p[kPMax * kPolyThreads];
  __shared__ D2 s_t[kTmpMax * kPolyThreads];
  __shared__ PolyBox s_gt[kEvalChunk];
  __shared__ uint32_t s_lo, s_hi;
  const int tid = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kPolyThreads + tid;
  const uint32_t key = q < D ? gkey_s[q] : kNoGroup;
  const bool real = key < groups;                                   // (padding rows sort behind every group)
  int32_t p = 0;
  uint32_t g0 = 0, g1 = 0;
  const double* bb = det_polys;
  double px1 = 0, py1 = 0, px2 = 0, py2 = 0;
  if (real) {
    p = grp_rank[q];
    g0 = gt_off[key];
    g1 = gt_off[key + 1];
    bb = det_polys + 8 * (int64_t)order[p];
    px1 = fmin(fmin(bb[0], bb[2]), fmin(bb[4], bb[6])); py1 = fmin(fmin(bb[1], bb[3]), fmin(bb[5], bb[7]));
    px2 = fmax(fmax(bb[0], bb[2]), fmax(bb[4], bb[6])); py2 = fmax(fmax(bb[1], bb[3]), fmax(bb[5], bb[7]));
  }
  // sorted keys: the first row holds the range's start, the last real row its end (no real first row: no real row at all)
  if (tid == 0) {
    s_lo = g0;
    if (!real) s_hi = 0;
  }
  if (real && (tid == kPolyThreads - 1 || q + 1 >= D || gkey_s[q + 1] >= groups)) s_hi = g1;
  __syncthreads();
  const uint32_t lo = s_lo, hi = s_hi;
  double best = -INFINITY;
  int32_t arg = -1;
  for (uint32_t c0 = lo; c0 < hi; c0 += kEvalChunk) {
    const uint32_t c1 = min(c0 + (uint32_t)kEvalChunk, hi);
    const bool need = real && g0 < c1 && g1 > c0;
    if (!__syncthreads_or(need)) continue;                          // (uniform; the barrier: the chunk before has been read)
    if (c0 + tid < c1) {
      const double* gt = gt_polys + 8 * (int64_t)gt_order[c0 + tid];
      PolyBox b;
#pragma unroll
      for (int k = 0; k < 8; k++) b.c[k] = gt[k];
      b.x1 = fmin(fmin(b.c[0], b.c[2]), fmin(b.c[4], b.c[6])); b.y1 = fmin(fmin(b.c[1], b.c[3]), fmin(b.c[5], b.c[7]));
      b.x2 = fmax(fmax(b.c[0], b.c[2]), fmax(b.c[4], b.c[6])); b.y2 = fmax(fmax(b.c[1], b.c[3]), fmax(b.c[5], b.c[7]));
      s_gt[tid] = b;
    }
    __syncthreads();
    if (need) {
      const int ja = (int)(max(g0, c0) - c0), jb = (int)(min(g1, c1) - c0);
      unsigned long long mask = 0;
      for (int j = ja; j < jb; j++) {
        const PolyBox& g = s_gt[j];
        const double iw = fmax(fmin(g.x2, px2) - fmax(g.x1, px1) + 1.0, 0.0);
        const double ih = fmax(fmin(g.y2, py2) - fmax(g.y1, py1) + 1.0, 0.0);
        const double inters = iw * ih;
        const double uni = (px2 - px1 + 1.0) * (py2 - py1 + 1.0) + (g.x2 - g.x1 + 1.0) * (g.y2 - g.y1 + 1.0) - inters;
        if (inters / uni > 0) mask |= 1ull << j;                    // :244
      }
      while (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const double ov = poly_iou(s_gt[j].c, bb, s_p + tid, s_t + tid);   // iou_poly(GT, bb), :250
        if (arg < 0 || ov > best) { best = ov; arg = (int32_t)(c0 + j); }
      }
    }
  }
  if (!real) return;
  ov_ws[p] = best;
  slot_ws[p] = arg;
  if (best > ovthresh && !(filter_difficult && gt_difficult[gt_order[arg]])) atomicMin(claim + arg, p);
}

// ---------------------------------------------------------------- tp / fp and their running counts
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, unsigned lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o);
    if (lane >= (unsigned)o) v += t;
  }
  return v;
}

// bit 0: TP, bit 1: FP (:265-290); a match with a filtered difficult box is neither; rows behind the real ones: 0
__global__ __launch_bounds__(256) void k_eval_mark(const double* __restrict__ ov_ws, const int32_t* __restrict__ slot_ws,
                                                   const int32_t* __restrict__ claim, const int32_t* __restrict__ gt_order,
                                                   const uint8_t* __restrict__ gt_difficult,
                                                   const uint32_t* __restrict__ seg_start, int32_t C, int64_t D,
                                                   double ovthresh, int filter_difficult, uint8_t* __restrict__ flag,
                                                   uint2* __restrict__ tile_tot) {
  __shared__ uint32_t s_tp[4], s_fp[4];
  const int64_t n = seg_start[C];
  const int64_t p0 = (int64_t)blockIdx.x * kEvalScanTile;
  uint32_t tp = 0, fp = 0;
  for (int k = 0; k < kEvalScanTile / 256; k++) {
    const int64_t p = p0 + k * 256 + threadIdx.x;
    if (p >= D) break;
    uint8_t f = 0;
    if (p < n) {
      if (ov_ws[p] > ovthresh) {
        const int32_t slot = slot_ws[p];
        if (!(filter_difficult && gt_difficult[gt_order[slot]])) f = claim[slot] == (int32_t)p ? 1 : 2;
      } else {
        f = 2;
      }
    }
    flag[p] = f;
    tp += f & 1u;
    fp += f >> 1;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    tp += (uint32_t)__shfl_xor((int)tp, o);
    fp += (uint32_t)__shfl_xor((int)fp, o);
  }
  if ((threadIdx.x & 63) == 0) { s_tp[threadIdx.x >> 6] = tp; s_fp[threadIdx.x >> 6] = fp; }
  __syncthreads();
  if (threadIdx.x == 0) tile_tot[blockIdx.x] = make_uint2(s_tp[0] + s_tp[1] + s_tp[2] + s_tp[3], s_fp[0] + s_fp[1] + s_fp[2] + s_fp[3]);
}

__device__ __forceinline__ uint2 block_scan_incl_1024(uint32_t a, uint32_t b, uint32_t* s_a, uint32_t* s_b) {
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  a = wave_scan_incl(a, lane);
  b = wave_scan_incl(b, lane);
  __syncthreads();                                                  // (s_a / s_b may still be read from the previous use)
  if (lane == 63) { s_a[wave] = a; s_b[wave] = b; }
  __syncthreads();
  for (unsigned w = 0; w < wave; w++) { a += s_a[w]; b += s_b[w]; }
  return make_uint2(a, b);
}

// one workgroup: tile totals -> exclusive prefix, in place
__global__ __launch_bounds__(1024) void k_eval_tile_scan(uint2* __restrict__ tile_tot, int64_t nb) {
  __shared__ uint32_t s_a[16], s_b[16];
  uint32_t ca = 0, cb = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
    const int64_t b = b0 + threadIdx.x;
    const uint2 v = b < nb ? tile_tot[b] : make_uint2(0u, 0u);
    const uint2 inc = block_scan_incl_1024(v.x, v.y, s_a, s_b);
    if (b < nb) tile_tot[b] = make_uint2(ca + inc.x - v.x, cb + inc.y - v.y);
    uint32_t ta = 0, tb = 0;
    for (int w = 0; w < 16; w++) { ta += s_a[w]; tb += s_b[w]; }
    ca += ta;
    cb += tb;
  }
}

// cum[p] = (TPs, FPs) at ranks <= p, over all classes: a class's own counts are cum[p] - cum[seg_start[c] - 1]
__global__ __launch_bounds__(1024) void k_eval_cum(const uint8_t* __restrict__ flag, const uint2* __restrict__ tile_base, int64_t D,
                                                   uint2* __restrict__ cum) {
  __shared__ uint32_t s_a[16], s_b[16];
  const int64_t p = (int64_t)blockIdx.x * kEvalScanTile + threadIdx.x;
  const uint32_t f = p < D ? flag[p] : 0u;
  const uint2 inc = block_scan_incl_1024(f & 1u, f >> 1, s_a, s_b);
  const uint2 base = tile_base[blockIdx.x];
  if (p < D) cum[p] = make_uint2(base.x + inc.x, base.y + inc.y);
}

// ---------------------------------------------------------------- per class
struct EvalOut {
  double *ap, *precision, *recall, *f1, *conf;
  long long *num_det_at_f1, *npos, *ndet;
  uint8_t* valid;
  long long *order, *argmax, *tp_cum, *fp_cum, *seg_start;      // optional curves (NULL: not wanted)
  double *ovmax, *rec, *prec;
};

struct ClassAcc {
  double area;         // area rule :83-88
  double p11[11];      // max(prec[rec >= t]) of :65-69 (0 when no position has rec >= t)
  double best_f1;
  uint32_t best_i;     // first maximum of f1, position inside the class
  uint32_t npos;
};

// One workgroup of 1 024 per class, walking the class segment from its END in steps of 4 096 positions (four consecutive
// ones per thread) with three carries: the maximum of prec behind the step (mpre of :79-80), the area sum, the best F1 so
// far.  Sums: a thread's positions in order, butterfly inside a wave, waves in order, steps in order -- one fixed order.
// rec is non-decreasing, so "rec >= t" (:66-69) is a suffix and max(prec[rec >= t]) is the suffix maximum at its first
// position.
__global__ __launch_bounds__(1024) void k_eval_class(const uint2* __restrict__ cum, const uint32_t* __restrict__ seg_start,
                                                     const uint32_t* __restrict__ gt_off, const int32_t* __restrict__ gt_order,
                                                     const uint8_t* __restrict__ gt_difficult, int32_t I, int filter_difficult,
                                                     EvalT11 t11, ClassAcc* __restrict__ acc) {
  __shared__ double s_wmax[16], s_wsum[16], s_wf1[16], s_p11[11], s_t11[11];
  __shared__ uint32_t s_wcnt[16], s_wf1i[16];
  const int c = blockIdx.x, tid = threadIdx.x;
  const unsigned lane = tid & 63, wave = tid >> 6;
  const uint32_t s = seg_start[c], n = seg_start[c + 1] - s;
  // npos: the ground truths of the class that count (:142-143 / :149: every box when difficult ones are not filtered)
  uint32_t cnt = 0;
  for (uint32_t g = gt_off[(uint32_t)c * I] + tid, g1 = gt_off[(uint32_t)(c + 1) * I]; g < g1; g += 1024)
    cnt += (!filter_difficult || !gt_difficult[gt_order[g]]) ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, o);
  if (lane == 0) s_wcnt[wave] = cnt;
  if (tid < 11) { s_p11[tid] = 0.0; s_t11[tid] = t11.t[tid]; }
  __syncthreads();
  uint32_t npos = 0;
  for (int w = 0; w < 16; w++) npos += s_wcnt[w];
  const double dpos = (double)npos;
  const uint2 base = s ? cum[s - 1] : make_uint2(0u, 0u);
  double carry_max = 0.0;                                           // mpre's closing 0.0 (:75)
  double area = 0.0, best_f1 = -1.0;                                // (thread 0)
  uint32_t best_i = 0;
  const uint32_t tiles = (n + kEvalClassTile - 1) / kEvalClassTile;
  for (uint32_t tile = tiles; tile-- > 0;) {
    const uint32_t i0 = tile * kEvalClassTile + tid * kEvalPerThread;   // this thread's kEvalPerThread consecutive positions
    double rec[kEvalPerThread], prec[kEvalPerThread], m[kEvalPerThread];
    double rec_left = 0.0;                                          // rec in front of i0 (mrec's opening 0.0 at the class's start)
    if (i0 > 0 && i0 < n && npos) rec_left = (double)(cum[s + i0 - 1].x - base.x) / dpos;
    double wf = -1.0;
    uint32_t wi = i0;
#pragma unroll
    for (int e = 0; e < kEvalPerThread; e++) {
      rec[e] = prec[e] = 0.0;
      if (i0 + e < n) {
        const uint2 v = cum[s + i0 + e];
        const double tp = (double)(v.x - base.x), fp = (double)(v.y - base.y);
        rec[e] = npos ? tp / dpos : 0.0;                            // :306
        prec[e] = tp / fmax(tp + fp, DBL_EPSILON);                  // :309
        const double f1 = 2.0 * rec[e] * prec[e] / (rec[e] + prec[e] + 1e-16);   // val.py:357
        if (f1 > wf) { wf = f1; wi = i0 + e; }                      // (first maximum: ascending e, strict >)
      }
    }
    // suffix maximum of prec (prec >= 0: 0.0 is neutral): inside the thread, then the threads behind it in the wave
    m[kEvalPerThread - 1] = prec[kEvalPerThread - 1];
#pragma unroll
    for (int e = kEvalPerThread - 2; e >= 0; e--) m[e] = fmax(prec[e], m[e + 1]);
    double sc = m[0];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double t = __shfl_down(sc, o);
      if (lane + o < 64) sc = fmax(sc, t);
    }
    double behind = __shfl_down(sc, 1);
    if (lane == 63) behind = 0.0;
    // first maximum of f1 inside the wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double of = __shfl_xor(wf, o);
      const uint32_t oi = (uint32_t)__shfl_xor((int)wi, o);
      if (of > wf || (of == wf && oi < wi)) { wf = of; wi = oi; }
    }
    __syncthreads();                                                // (the step before this one has been read)
    if (lane == 0) { s_wmax[wave] = sc; s_wf1[wave] = wf; s_wf1i[wave] = wi; }
    __syncthreads();
    double all = carry_max;
    behind = fmax(behind, carry_max);                               // ... the waves behind this one, the steps behind this one
    for (unsigned w = 0; w < 16; w++) {
      const double mw = s_wmax[w];
      all = fmax(all, mw);
      if (w > wave) behind = fmax(behind, mw);
    }
    carry_max = all;
    // area rule :83-88: the positions where mrec changes, times mpre there; 11-point rule :65-70: the first position with
    // rec >= t
    double term = 0.0;
#pragma unroll
    for (int e = 0; e < kEvalPerThread; e++) {
      const double suf = fmax(m[e], behind), prev = e ? rec[e - 1] : rec_left;
      if (i0 + e < n) {
        if (rec[e] != prev) term += (rec[e] - prev) * suf;
#pragma unroll 1
        for (int k = 0; k < 11; k++) {
          const double t = s_t11[k];
          if (rec[e] >= t && (i0 + e == 0 || !(prev >= t))) s_p11[k] = suf;
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
    if (lane == 0) s_wsum[wave] = term;
    __syncthreads();
    if (tid == 0) {
      double ts = 0.0;
      for (int w = 0; w < 16; w++) ts += s_wsum[w];
      area += ts;
      for (int w = 0; w < 16; w++) {
        const double f = s_wf1[w];
        const uint32_t fi = s_wf1i[w];
        if (f > best_f1 || (f == best_f1 && fi < best_i)) { best_f1 = f; best_i = fi; }
      }
    }
  }
  if (tid < 11) acc[c].p11[tid] = s_p11[tid];
  if (tid != 0) return;
  acc[c].area = area;
  acc[c].best_f1 = best_f1;
  acc[c].best_i = best_i;
  acc[c].npos = npos;
}

// the per-class outputs out of the class accumulators, and the optional curves: one value per position of the order, every
// curve array cleared behind the last real detection
__global__ void k_eval_finish(const ClassAcc* __restrict__ acc, const uint2* __restrict__ cum, const int32_t* __restrict__ order,
                              const double* __restrict__ det_scores, const double* __restrict__ ov_ws,
                              const int32_t* __restrict__ slot_ws, const int32_t* __restrict__ gt_order,
                              const uint32_t* __restrict__ seg_start, int32_t C, int64_t D, int use_07_metric, int want_curves,
                              EvalOut out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < C) {
    const int c = (int)p;
    const uint32_t s = seg_start[c], n = seg_start[c + 1] - s, npos = acc[c].npos;
    out.npos[c] = (long long)npos;
    out.ndet[c] = (long long)n;
    out.valid[c] = npos ? 1 : 0;
    if (n == 0 || npos == 0) {                                      // :322 / a class without countable ground truth
      out.ap[c] = out.precision[c] = out.recall[c] = out.f1[c] = out.conf[c] = 0.0;
      out.num_det_at_f1[c] = 0;
    } else {
      double ap = acc[c].area;
      if (use_07_metric) {
        ap = 0.0;
        for (int k = 0; k < 11; k++) ap = ap + acc[c].p11[k] / 11.0;   // :70, in t order
      }
      const uint32_t bi = acc[c].best_i;
      const uint2 base = s ? cum[s - 1] : make_uint2(0u, 0u), v = cum[s + bi];
      const double tp = (double)(v.x - base.x), fp = (double)(v.y - base.y);
      out.ap[c] = ap;
      out.precision[c] = tp / fmax(tp + fp, DBL_EPSILON);
      out.recall[c] = tp / (double)npos;
      out.f1[c] = acc[c].best_f1;
      out.conf[c] = det_scores[order[s + bi]];
      out.num_det_at_f1[c] = (long long)bi + 1;
    }
  }
  if (!want_curves) return;
  if (out.seg_start && p <= C) out.seg_start[p] = seg_start[p];
  if (p >= D) return;
  const bool real = p < (int64_t)seg_start[C];
  if (out.order) out.order[p] = real ? order[p] : -1;
  if (out.ovmax) out.ovmax[p] = real ? ov_ws[p] : 0.0;
  if (out.argmax) {
    const int32_t slot = real ? slot_ws[p] : -1;
    out.argmax[p] = slot >= 0 ? gt_order[slot] : -1;
  }
  long long tpc = 0, fpc = 0;
  double rec = 0.0, prec = 0.0;
  if (real) {
    int lo = 0, hi = C;                                             // the class of p: last c with seg_start[c] <= p
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((int64_t)seg_start[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t s = seg_start[lo], npos = acc[lo].npos;
    const uint2 base = s ? cum[s - 1] : make_uint2(0u, 0u), v = cum[p];
    const double tp = (double)(v.x - base.x), fp = (double)(v.y - base.y);
    tpc = (long long)(v.x - base.x);
    fpc = (long long)(v.y - base.y);
    rec = npos ? tp / (double)npos : 0.0;                           // :306
    prec = tp / fmax(tp + fp, DBL_EPSILON);                         // :309
  }
  if (out.tp_cum) out.tp_cum[p] = tpc;
  if (out.fp_cum) out.fp_cum[p] = fpc;
  if (out.rec) out.rec[p] = rec;
  if (out.prec) out.prec[p] = prec;
}

size_t eval_sort_scratch(size_t n) { return n * 40 + (8u << 20); }
struct EvalWs {                                       // carved from the workspace, in this order
  unsigned long long *key_a, *key_s; int32_t *idx_a, *ord1; uint32_t *ckey_a, *ckey_s; int32_t* order; uint32_t *gkey_a, *gkey_s;
  int32_t *rank_a, *grp_rank; double* ov_ws; uint2* cum; uint8_t* flag;                      // [D] each
  uint2* tile_tot;                                                                           // [D / kEvalScanTile, rounded up]
  uint32_t *gtkey_a, *gtkey_s; int32_t *gtidx_a, *gt_order, *claim;                          // [G] each
  uint32_t *gt_off, *seg_start; ClassAcc* acc;                                               // [groups + 1], [kEvalMaxClasses + 2], [kEvalMaxClasses]
  void* rp; size_t rpb;                                                                      // rocPRIM sort scratch, its bytes
};
bool carve(Carver& cv, size_t D, size_t G, size_t groups, EvalWs& w) {
  w.key_a = cv.take<unsigned long long>(D);
  w.key_s = cv.take<unsigned long long>(D);
  w.idx_a = cv.take<int32_t>(D);
  w.ord1 = cv.take<int32_t>(D);
  w.ckey_a = cv.take<uint32_t>(D);
  w.ckey_s = cv.take<uint32_t>(D);
  w.order = cv.take<int32_t>(D);
  w.gkey_a = cv.take<uint32_t>(D);
  w.gkey_s = cv.take<uint32_t>(D);
  w.rank_a = cv.take<int32_t>(D);
  w.grp_rank = cv.take<int32_t>(D);
  w.ov_ws = cv.take<double>(D);
  w.cum = cv.take<uint2>(D);
  w.flag = cv.take<uint8_t>(D);
  w.tile_tot = cv.take<uint2>((D + kEvalScanTile - 1) / kEvalScanTile);
  w.gtkey_a = cv.take<uint32_t>(G);
  w.gtkey_s = cv.take<uint32_t>(G);
  w.gtidx_a = cv.take<int32_t>(G);
  w.gt_order = cv.take<int32_t>(G);
  w.claim = cv.take<int32_t>(G);
  w.gt_off = cv.take<uint32_t>(groups + 1);
  w.seg_start = cv.take<uint32_t>(kEvalMaxClasses + 2);
  w.acc = cv.take<ClassAcc>(kEvalMaxClasses);
  w.rpb = eval_sort_scratch(std::max(D, G));
  w.rp = cv.take<char>(w.rpb);
  return cv.ok();
}
constexpr size_t kEvalWsSlack = 4096;   // headroom the query has always declared; no sub-buffer lives in it
// keys / vals [n] sorted by bits [0, bits) of the key into keys_out / vals_out, on the carved scratch
template <typename K>
int eval_sort(const EvalWs& w, K* keys, K* keys_out, int32_t* vals, int32_t* vals_out, size_t n, int bits, hipStream_t st) {
  size_t need = 0;
  S2A_HIP(rocprim::radix_sort_pairs(nullptr, need, keys, keys_out, vals, vals_out, n, 0, bits, st));
  if (need > w.rpb) {
    set_error("eval_task1: workspace too small (sort scratch %zu < %zu bytes)", w.rpb, need);
    return S2A_EWORKSPACE;
  }
  S2A_HIP(rocprim::radix_sort_pairs(w.rp, need, keys, keys_out, vals, vals_out, n, 0, bits, st));
  return S2A_OK;
}

int bits_for(uint64_t max_value) {
  int b = 1;
  while (b < 64 && (max_value >> b) != 0) b++;
  return b;
}

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" size_t s2a_eval_task1_workspace_bytes(int64_t num_dets, int64_t num_gts, int32_t num_classes, int32_t num_images) {
  if (num_dets < 0 || num_gts < 0 || num_dets >= (1ll << 31) || num_gts >= (1ll << 31) || num_classes < 1 ||
      num_classes > kEvalMaxClasses || num_images < 1 || ((int64_t)num_classes + 1) * num_images >= (1ll << 31))
    return 0;   // (sizes the entry point refuses)
  return carved_bytes<EvalWs>((size_t)num_dets, (size_t)num_gts, (size_t)num_classes * (size_t)num_images) + kEvalWsSlack;
}

extern "C" int s2a_eval_task1(const double* det_polys, const double* det_scores, const int32_t* det_labels,
                              const int32_t* det_image, int64_t num_dets, const double* gt_polys, const int32_t* gt_labels,
                              const int32_t* gt_image, const uint8_t* gt_difficult, int64_t num_gts, int32_t num_classes,
                              int32_t num_images, double ovthresh, int is_filter_difficult, int use_07_metric,
                              const double* thresholds11, double* ap, double* precision, double* recall, double* f1,
                              double* conf, int64_t* num_det_at_f1, int64_t* npos, int64_t* ndet, uint8_t* valid,
                              const s2a_eval_curves* curves, void* workspace, size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(num_dets >= 0 && num_gts >= 0, "eval_task1: negative size");
  S2A_CHECK_ARG(num_dets < (1ll << 31) && num_gts < (1ll << 31), "eval_task1: 2^31 rows or more are not supported");
  S2A_CHECK_ARG(num_classes >= 1 && num_classes <= kEvalMaxClasses, "eval_task1: num_classes must be in [1, 1024]");
  S2A_CHECK_ARG(num_images >= 1 && ((int64_t)num_classes + 1) * num_images < (1ll << 31),
                "eval_task1: num_images must be >= 1 and (num_classes + 1) * num_images < 2^31");
  S2A_CHECK_ARG(ap && precision && recall && f1 && conf && num_det_at_f1 && npos && ndet && valid, "eval_task1: NULL output");
  S2A_CHECK_ARG(num_dets == 0 || (det_polys && det_scores && det_labels && det_image), "eval_task1: NULL detection tensor");
  S2A_CHECK_ARG(num_gts == 0 || (gt_polys && gt_labels && gt_image && gt_difficult), "eval_task1: NULL ground-truth tensor");
  S2A_CHECK_ARG(thresholds11 || !use_07_metric, "eval_task1: the 11-point rule needs its 11 recall thresholds");
  const int64_t D = num_dets, G = num_gts;
  const int32_t C = num_classes, I = num_images;
  const size_t szD = (size_t)D, szG = (size_t)G, groups = (size_t)C * (size_t)I;
  const size_t nb = (szD + kEvalScanTile - 1) / kEvalScanTile;
  hipStream_t st = as_stream(stream);
  EvalWs w;
  if (int rc = carve_workspace(workspace, workspace_bytes, w, kEvalWsSlack, "eval_task1", szD, szG, groups)) return rc;
  int32_t* slot_ws = w.idx_a;                                        // (idx_a is free once the first sort has run)
  const int cbits = bits_for((uint64_t)C), gbits = bits_for((uint64_t)groups);
  if (D > 0) {
    const unsigned gd = (unsigned)((D + 255) / 256);
    k_eval_det_keys<<<gd, 256, 0, st>>>(det_scores, det_labels, det_image, D, C, I, w.key_a, w.idx_a);
    if (int rc = eval_sort(w, w.key_a, w.key_s, w.idx_a, w.ord1, szD, 64, st)) return rc;
    k_eval_class_keys<<<gd, 256, 0, st>>>(w.ord1, det_labels, det_image, D, C, I, w.ckey_a);
    if (int rc = eval_sort(w, w.ckey_a, w.ckey_s, w.ord1, w.order, szD, cbits, st)) return rc;
    k_eval_group_keys<<<gd, 256, 0, st>>>(w.ckey_s, w.order, det_image, D, C, I, w.gkey_a, w.rank_a);
    if (int rc = eval_sort(w, w.gkey_a, w.gkey_s, w.rank_a, w.grp_rank, szD, gbits, st)) return rc;
  }
  if (G > 0) {
    k_eval_gt_keys<<<(unsigned)((G + 255) / 256), 256, 0, st>>>(gt_labels, gt_image, G, C, I, w.gtkey_a, w.gtidx_a);
    if (int rc = eval_sort(w, w.gtkey_a, w.gtkey_s, w.gtidx_a, w.gt_order, szG, gbits, st)) return rc;
  }
  const int64_t table_n = std::max<int64_t>((int64_t)groups + 1, G);
  k_eval_tables<<<(unsigned)((table_n + 255) / 256), 256, 0, st>>>(w.gtkey_s, G, w.ckey_s, D, C, I, w.gt_off, w.seg_start, w.claim);
  EvalOut out = {};
  out.ap = ap; out.precision = precision; out.recall = recall; out.f1 = f1; out.conf = conf;
  out.num_det_at_f1 = reinterpret_cast<long long*>(num_det_at_f1);
  out.npos = reinterpret_cast<long long*>(npos);
  out.ndet = reinterpret_cast<long long*>(ndet);
  out.valid = valid;
  bool want_curves = false;
  if (curves) {
    out.order = reinterpret_cast<long long*>(curves->order);
    out.argmax = reinterpret_cast<long long*>(curves->argmax);
    out.tp_cum = reinterpret_cast<long long*>(curves->tp_cum);
    out.fp_cum = reinterpret_cast<long long*>(curves->fp_cum);
    out.seg_start = reinterpret_cast<long long*>(curves->seg_start);
    out.ovmax = curves->ovmax; out.rec = curves->rec; out.prec = curves->prec;
    want_curves = out.order || out.argmax || out.tp_cum || out.fp_cum || out.seg_start || out.ovmax || out.rec || out.prec;
  }
  if (D > 0) {
    k_eval_match<<<(unsigned)((D + kPolyThreads - 1) / kPolyThreads), kPolyThreads, 0, st>>>(
        w.gkey_s, w.grp_rank, w.order, D, det_polys, gt_polys, w.gt_order, gt_difficult, w.gt_off, (uint32_t)groups, ovthresh,
        is_filter_difficult, w.ov_ws, slot_ws, w.claim);
    k_eval_mark<<<(unsigned)nb, 256, 0, st>>>(w.ov_ws, slot_ws, w.claim, w.gt_order, gt_difficult, w.seg_start, C, D, ovthresh,
                                               is_filter_difficult, w.flag, w.tile_tot);
    k_eval_tile_scan<<<1, 1024, 0, st>>>(w.tile_tot, (int64_t)nb);
    k_eval_cum<<<(unsigned)nb, 1024, 0, st>>>(w.flag, w.tile_tot, D, w.cum);
  }
  EvalT11 t11;
  for (int k = 0; k < 11; k++) t11.t[k] = thresholds11 ? thresholds11[k] : 0.1 * k;
  k_eval_class<<<(unsigned)C, 1024, 0, st>>>(w.cum, w.seg_start, w.gt_off, w.gt_order, gt_difficult, I, is_filter_difficult, t11, w.acc);
  const int64_t fn = std::max<int64_t>(want_curves ? D : 0, (int64_t)C + 1);
  k_eval_finish<<<(unsigned)((fn + 255) / 256), 256, 0, st>>>(w.acc, w.cum, w.order, det_scores, w.ov_ws, slot_ws, w.gt_order, w.seg_start, C, D,
                                                              use_07_metric, want_curves ? 1 : 0, out);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
