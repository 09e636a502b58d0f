// Training-mode BatchNorm (bn_ops.hip): the slice plan of the four passes, the per-lane moment accumulator and the merges.
// Plain C++: included by the kernels and by tests/bn_plan_walk.cpp, which walks the same arithmetic on the CPU.
//
// The activation is f16 channels-last seen as [P, C], C % 64 == 0.  A workgroup of 256 threads owns one GROUP of 64 channels
// and one SLICE of rows; thread (cx = tid & 7, ry = tid >> 3) keeps the channel octet cx of the group for the whole walk and
// takes rows r0 + ry, r0 + ry + 32, ... of the slice.  groups x slices workgroups; both follow from (P, C) alone.
// A slice is a run of whole 32-row tiles; slices past the last tile are EMPTY: they write identities (count 0).
//
// Moments: a lane accumulates sum(x - K) and sum((x - K)^2) in f32 around K = its own first value (the shifted-data form:
// what cancels is (mean - K)^2 against the variance, not mean^2), and hands on (count, mean, M2).  Groups of such triples are
// merged in double by the pairwise-update formula of Chan, Golub & LeVeque (1979) in its k-way form:
//     n = sum n_i,   mean = sum n_i mean_i / n,   M2 = sum (M2_i + n_i (mean_i - mean)^2),
// lanes in lane order inside the workgroup; in the finalise launch sixteen threads per channel each merge every sixteenth
// slice in slice order, and their results are merged in thread order.  Counts are never stored: they follow from the plan.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define S2A_BN_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define S2A_BN_HD inline
#endif

namespace s2a {
namespace bn {

constexpr int kRowLanes = 32;      // rows a workgroup takes per step (256 threads / 8 octets)
constexpr int kGroup = 64;         // channels of a workgroup
constexpr int kMaxSlices = 256;
constexpr int kBlocksAim = 1024;   // groups x slices aims at this many workgroups

struct Plan {
  int64_t P;                       // positions
  int64_t rows_per_slice;          // a multiple of kRowLanes
  int C, groups, slices;
};

// what the kernels handle: at least two positions (the unbiased variance), whole 64-channel groups, under 2^31 bytes
S2A_BN_HD bool plan_ok(int64_t P, int64_t C) {
  return P >= 2 && C > 0 && C % kGroup == 0 && C < (1ll << 24) && P < (1ll << 31) && (uint64_t)P * (uint64_t)C * 2 < (1ull << 31);
}

S2A_BN_HD int plan_slices(int64_t P, int64_t C) {
  if (!plan_ok(P, C)) return 0;
  const int64_t groups = C / kGroup;
  int64_t s = kBlocksAim / groups;
  s = s < 1 ? 1 : s;
  return (int)(s > kMaxSlices ? kMaxSlices : s);
}

S2A_BN_HD Plan make_plan(int64_t P, int64_t C) {
  Plan pl;
  pl.P = P;
  pl.C = (int)C;
  pl.groups = (int)(C / kGroup);
  pl.slices = plan_slices(P, C);
  const int64_t tiles = (P + kRowLanes - 1) / kRowLanes;
  pl.rows_per_slice = (tiles + pl.slices - 1) / pl.slices * kRowLanes;
  return pl;
}

// rows [r0, r1) of slice s; r0 == r1 for an empty slice
S2A_BN_HD void slice_rows(const Plan& pl, int s, int64_t& r0, int64_t& r1) {
  r0 = (int64_t)s * pl.rows_per_slice;
  r1 = r0 + pl.rows_per_slice;
  if (r0 > pl.P) r0 = pl.P;
  if (r1 > pl.P) r1 = pl.P;
}

// how many rows lane ry takes of [r0, r1): r0 + ry, r0 + ry + 32, ...
S2A_BN_HD int64_t lane_rows(int64_t r0, int64_t r1, int ry) {
  const int64_t first = r0 + ry;
  return first >= r1 ? 0 : (r1 - first + kRowLanes - 1) / kRowLanes;
}

// one lane, one channel
struct LaneAcc {
  float K, s1, s2;
  // the first value: the shift when it is finite (then s1 = s2 = 0 exactly); an inf or NaN is summed around 0 instead, so that
  // a +-inf gives mean +-inf and M2 NaN wherever it stands in the lane, as the two-pass definition does
  S2A_BN_HD void start(float x) {
    K = (x - x == 0.f) ? x : 0.f;
    s1 = x - K;
    s2 = s1 * s1;
  }
  S2A_BN_HD void add(float x) {
    const float d = x - K;
    s1 += d;
    s2 += d * d;
  }
  // n >= 1 values seen (start counts as one) -> mean and M2 = sum (x - mean)^2; a NaN stays a NaN
  S2A_BN_HD void finish(int64_t n, float& mean, float& m2) const {
    const float inv = 1.f / (float)n;
    mean = K + s1 * inv;
    const float v = s2 - s1 * s1 * inv;
    m2 = v < 0.f ? 0.f : v;
  }
};

struct LaneCounts {
  int64_t r0, r1;
  S2A_BN_HD int64_t operator()(int q) const { return lane_rows(r0, r1, q); }
};
struct SliceCounts {
  Plan pl;
  S2A_BN_HD int64_t operator()(int s) const {
    int64_t r0, r1;
    slice_rows(pl, s, r0, r1);
    return r1 - r0;
  }
};

struct StridedCounts {
  const int64_t* n;
  int stride;
  S2A_BN_HD int64_t operator()(int i) const { return n[i * stride]; }
};

#if defined(__HIPCC__)
#define S2A_BN_UNROLL _Pragma("unroll 8")
#else
#define S2A_BN_UNROLL
#endif

// k-way merge of the members i = first, first + step, ... < k, in that order, of (count(i), mean[i * stride], m2[i * stride]);
// members of count 0 take no part whatever they hold (selected away, not branched over: the loads of a trip do not wait for
// the trip before).  -> total count (0: mean = M2 = 0)
template <typename T, typename Counts>
S2A_BN_HD int64_t merge_moments(const T* mean, const T* m2, int64_t stride, int first, int step, int k, const Counts& count,
                                double& mean_out, double& m2_out) {
  int64_t n = 0;
  double sum = 0.0;
  S2A_BN_UNROLL
  for (int i = first; i < k; i += step) {
    const int64_t ni = count(i);
    const double mi = (double)mean[i * stride];
    n += ni;
    sum += ni ? (double)ni * mi : 0.0;
  }
  mean_out = 0.0;
  m2_out = 0.0;
  if (n == 0) return 0;
  const double mu = sum / (double)n;
  double acc = 0.0;
  S2A_BN_UNROLL
  for (int i = first; i < k; i += step) {
    const int64_t ni = count(i);
    const double d = (double)mean[i * stride] - mu, qi = (double)m2[i * stride];
    acc += ni ? qi + (double)ni * d * d : 0.0;
  }
  mean_out = mu;
  m2_out = acc;
  return n;
}

// the finalise launch: kFinalLanes threads per channel.  Lane q merges the slices q, q + kFinalLanes, ... (final_lane); the
// lanes' (count, mean, M2), held in double, are merged in lane order (final_all)
constexpr int kFinalLanes = 16;

S2A_BN_HD int64_t final_lane(const Plan& pl, const float* partial, int c, int q, double& mean_out, double& m2_out) {
  return merge_moments(partial + c, partial + pl.C + c, (int64_t)2 * pl.C, q, kFinalLanes, pl.slices, SliceCounts{pl}, mean_out, m2_out);
}

S2A_BN_HD int64_t final_all(const double* mean, const double* m2, const int64_t* n, int stride, double& mean_out, double& m2_out) {
  return merge_moments(mean, m2, (int64_t)stride, 0, 1, kFinalLanes, StridedCounts{n, stride}, mean_out, m2_out);
}

}  // namespace bn
}  // namespace s2a
