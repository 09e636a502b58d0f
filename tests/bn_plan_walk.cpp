// Walks the slice plan of the training-mode BatchNorm kernels (s2anet_amd/csrc/bn_plan.hpp) on the CPU, through the very
// functions the kernels call, on exact-size heap buffers (built with -fsanitize=address,undefined by
// tests/test_batchnorm_cpu.py):
//   bn_plan_walk cover P C [P C ...]   every row and every channel of [P, C] is taken by exactly one (slice, lane) / (group,
//                                      octet), lane_rows() is the count the walk makes, `partial` is written completely and
//                                      only inside [slices][2][C]
//   bn_plan_walk identity              empty slices (and lanes without a row) merge as identities, whatever they hold
//   bn_plan_walk offset P C            channel means 8, std 1/16 on the f16 grid: lanes (f32, shifted sums) -> workgroup merge
//                                      -> slice merge equals the float64 two-pass mean / variance
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "bn_plan.hpp"

using namespace s2a::bn;

#define REQUIRE(cond, ...)                 \
  do {                                     \
    if (!(cond)) {                         \
      std::fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
      return 1;                            \
    }                                      \
  } while (0)

static int cover(int64_t P, int64_t C) {
  REQUIRE(plan_ok(P, C), "P %lld C %lld", (long long)P, (long long)C);
  const Plan pl = make_plan(P, C);
  REQUIRE(pl.slices == plan_slices(P, C) && pl.slices >= 1 && pl.slices <= kMaxSlices, "slices %d", pl.slices);
  REQUIRE(pl.groups * kGroup == C && pl.rows_per_slice % kRowLanes == 0 && pl.rows_per_slice > 0, "groups %d", pl.groups);
  std::vector<uint8_t> rows((size_t)P, 0), chans((size_t)C, 0), partial((size_t)pl.slices * 2 * (size_t)C, 0);
  int64_t total = 0, empty = 0;
  for (int s = 0; s < pl.slices; s++) {
    int64_t r0, r1;
    slice_rows(pl, s, r0, r1);
    REQUIRE(0 <= r0 && r0 <= r1 && r1 <= P, "slice %d rows [%lld, %lld)", s, (long long)r0, (long long)r1);
    empty += r0 == r1;
    for (int ry = 0; ry < kRowLanes; ry++) {
      int64_t n = 0;
      for (int64_t r = r0 + ry; r < r1; r += kRowLanes) {      // the kernels' walk
        rows[(size_t)r]++;
        n++;
      }
      REQUIRE(n == lane_rows(r0, r1, ry), "slice %d lane %d: walked %lld, lane_rows %lld", s, ry, (long long)n,
              (long long)lane_rows(r0, r1, ry));
      total += n;
    }
    for (int g = 0; g < pl.groups; g++)                         // what thread tid < 64 of workgroup (g, s) writes
      for (int t = 0; t < kGroup; t++) {
        const int64_t at = (int64_t)s * 2 * C + g * kGroup + t;
        partial.at((size_t)at)++;
        partial.at((size_t)(at + C))++;
      }
  }
  for (int g = 0; g < pl.groups; g++)
    for (int cx = 0; cx < 8; cx++)
      for (int j = 0; j < 8; j++) chans.at((size_t)(g * kGroup + cx * 8 + j))++;
  REQUIRE(total == P, "rows walked %lld of %lld", (long long)total, (long long)P);
  for (int64_t r = 0; r < P; r++) REQUIRE(rows[(size_t)r] == 1, "row %lld taken %d times", (long long)r, rows[(size_t)r]);
  for (int64_t c = 0; c < C; c++) REQUIRE(chans[(size_t)c] == 1, "channel %lld taken %d times", (long long)c, chans[(size_t)c]);
  for (size_t i = 0; i < partial.size(); i++) REQUIRE(partial[i] == 1, "partial[%zu] written %d times", i, partial[i]);
  std::printf("cover P %lld C %lld: groups %d slices %d rows_per_slice %lld tiles %lld empty_slices %lld\n", (long long)P,
              (long long)C, pl.groups, pl.slices, (long long)pl.rows_per_slice, (long long)((P + kRowLanes - 1) / kRowLanes),
              (long long)empty);
  return 0;
}

struct FixedCounts {
  const int64_t* n;
  int64_t operator()(int i) const { return n[i]; }
};

static int identity() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // three real members; the same three with empty ones in front, between and behind, holding zeros, NaN and inf
  const float mean3[3] = {8.25f, 7.9375f, 8.0f}, m23[3] = {0.5f, 0.25f, 0.f};
  const int64_t n3[3] = {32, 7, 1};
  double m_ref, q_ref;
  REQUIRE(merge_moments(mean3, m23, 1, 0, 1, 3, FixedCounts{n3}, m_ref, q_ref) == 40, "count");
  for (float filler : {0.f, nan, inf, -3.f}) {
    const float mean7[7] = {filler, 8.25f, filler, 7.9375f, 8.0f, filler, filler};
    const float m27[7] = {filler, 0.5f, filler, 0.25f, 0.f, filler, filler};
    const int64_t n7[7] = {0, 32, 0, 7, 1, 0, 0};
    double m, q;
    REQUIRE(merge_moments(mean7, m27, 1, 0, 1, 7, FixedCounts{n7}, m, q) == 40, "count with empty members");
    REQUIRE(std::memcmp(&m, &m_ref, 8) == 0 && std::memcmp(&q, &q_ref, 8) == 0, "filler %f: %.17g %.17g, want %.17g %.17g",
            (double)filler, m, q, m_ref, q_ref);
  }
  {   // every second member from the second on: members 1 and 3 only
    const float mean4[4] = {nan, 8.25f, inf, 7.9375f}, m24[4] = {nan, 0.5f, nan, 0.25f};
    const int64_t n4[4] = {5, 32, 9, 7}, n2[2] = {32, 7};
    const float mean2[2] = {8.25f, 7.9375f}, m22[2] = {0.5f, 0.25f};
    double ma, qa, mb, qb;
    REQUIRE(merge_moments(mean4, m24, 1, 1, 2, 4, FixedCounts{n4}, ma, qa) == 39, "strided count");
    REQUIRE(merge_moments(mean2, m22, 1, 0, 1, 2, FixedCounts{n2}, mb, qb) == 39 && ma == mb && qa == qb, "strided merge");
  }
  const int64_t none[2] = {0, 0};
  const float junk[2] = {nan, inf};
  double m, q;
  REQUIRE(merge_moments(junk, junk, 1, 0, 1, 2, FixedCounts{none}, m, q) == 0 && m == 0.0 && q == 0.0, "all empty");
  // the plan's own empty slices: [32, 2048] has one tile and many slices
  const Plan pl = make_plan(32, 2048);
  int64_t r0, r1;
  slice_rows(pl, 0, r0, r1);
  REQUIRE(r1 - r0 == 32, "first slice");
  for (int s = 1; s < pl.slices; s++) {
    slice_rows(pl, s, r0, r1);
    REQUIRE(r0 == r1 && SliceCounts{pl}(s) == 0, "slice %d is not empty", s);
  }
  // a lane with an inf: mean inf and M2 NaN whether the inf comes first or last; a finite lane is exact around its first value
  for (int first = 0; first < 2; first++) {
    LaneAcc acc;
    acc.start(first ? inf : 2.f);
    acc.add(3.f);
    acc.add(first ? 2.f : inf);
    float lm, lq;
    acc.finish(3, lm, lq);
    REQUIRE(lm == inf && lq != lq, "inf %s: mean %f M2 %f", first ? "first" : "last", (double)lm, (double)lq);
  }
  LaneAcc fin;
  fin.start(8.25f);
  fin.add(8.25f);
  float lm, lq;
  fin.finish(2, lm, lq);
  REQUIRE(lm == 8.25f && lq == 0.f, "constant lane: mean %f M2 %f", (double)lm, (double)lq);
  std::printf("identity ok\n");
  return 0;
}

static uint64_t lcg(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 33;
}
static double gauss(uint64_t& s) {      // Box-Muller
  const double u1 = ((double)lcg(s) + 1.0) / 2147483649.0, u2 = (double)lcg(s) / 2147483648.0;
  return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
}

static int offset(int64_t P, int64_t C) {
  REQUIRE(plan_ok(P, C), "P %lld C %lld", (long long)P, (long long)C);
  const Plan pl = make_plan(P, C);
  // mean 8, std 1/16, on the f16 grid (multiples of 2^-7 in [4, 16) are f16 numbers)
  std::vector<float> x((size_t)(P * C));
  uint64_t seed = 12345;
  for (auto& v : x) v = 8.f + (float)std::lrint(gauss(seed) * 8.0) / 128.f;
  std::vector<float> partial((size_t)pl.slices * 2 * (size_t)C, std::numeric_limits<float>::quiet_NaN());
  std::vector<float> s_mean((size_t)kRowLanes * kGroup), s_m2((size_t)kRowLanes * kGroup);
  for (int s = 0; s < pl.slices; s++)
    for (int g = 0; g < pl.groups; g++) {
      int64_t r0, r1;
      slice_rows(pl, s, r0, r1);
      for (int ry = 0; ry < kRowLanes; ry++)
        for (int c = 0; c < kGroup; c++) {                      // k_bn_stats, one lane and one of its channels
          LaneAcc acc;
          acc.start(0.f);
          int64_t r = r0 + ry;
          const int64_t n = lane_rows(r0, r1, ry);
          if (r < r1) {
            acc.start(x.at((size_t)(r * C + g * kGroup + c)));
            r += kRowLanes;
          }
          for (; r < r1; r += kRowLanes) acc.add(x.at((size_t)(r * C + g * kGroup + c)));
          float m = 0.f, q = 0.f;
          if (n > 0) acc.finish(n, m, q);
          s_mean.at((size_t)(ry * kGroup + c)) = m;
          s_m2.at((size_t)(ry * kGroup + c)) = q;
        }
      for (int t = 0; t < kGroup; t++) {
        double m, q;
        merge_moments(&s_mean[(size_t)t], &s_m2[(size_t)t], kGroup, 0, 1, kRowLanes, LaneCounts{r0, r1}, m, q);
        const int64_t at = (int64_t)s * 2 * C + g * kGroup + t;
        partial.at((size_t)at) = (float)m;
        partial.at((size_t)(at + C)) = (float)q;
      }
    }
  double worst_mean = 0, worst_var = 0, worst_naive = 0;
  for (int64_t c = 0; c < C; c++) {
    double m, q, lane_mean[kFinalLanes], lane_m2[kFinalLanes];      // k_bn_stats_final: sixteen lanes, then their merge
    int64_t lane_n[kFinalLanes];
    for (int lane = 0; lane < kFinalLanes; lane++)
      lane_n[lane] = final_lane(pl, partial.data(), (int)c, lane, lane_mean[lane], lane_m2[lane]);
    REQUIRE(final_all(lane_mean, lane_m2, lane_n, 1, m, q) == P, "count");
    double mu = 0, var = 0;
    for (int64_t r = 0; r < P; r++) mu += (double)x[(size_t)(r * C + c)];
    mu /= (double)P;
    for (int64_t r = 0; r < P; r++) var += ((double)x[(size_t)(r * C + c)] - mu) * ((double)x[(size_t)(r * C + c)] - mu);
    var /= (double)P;
    float s1 = 0.f, s2 = 0.f;                                   // for the record: the plain f32 form
    for (int64_t r = 0; r < P; r++) {
      s1 += x[(size_t)(r * C + c)];
      s2 += x[(size_t)(r * C + c)] * x[(size_t)(r * C + c)];
    }
    const float naive = s2 / (float)P - (s1 / (float)P) * (s1 / (float)P);
    worst_mean = std::fmax(worst_mean, std::fabs(m - mu) / std::fabs(mu));
    worst_var = std::fmax(worst_var, std::fabs(q / (double)P - var) / var);
    worst_naive = std::fmax(worst_naive, std::fabs((double)naive - var) / var);
  }
  std::printf("offset P %lld C %lld: mean rel err %.3e, variance rel err %.3e (plain f32 E[x^2] - mean^2: %.3e)\n", (long long)P,
              (long long)C, worst_mean, worst_var, worst_naive);
  // mean: f32 partial means (2^-24 each) merged in double; variance: f32 lane sums of a few terms around the lane's own first
  // value, (mean - K)^2 / var is O(1): a few 2^-24, 2^-20 leaves a factor 16
  REQUIRE(worst_mean <= std::ldexp(1.0, -23), "mean");
  REQUIRE(worst_var <= std::ldexp(1.0, -20), "variance");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "cover") && argc % 2 == 0) {
    for (int i = 2; i + 1 < argc; i += 2)
      if (cover(std::atoll(argv[i]), std::atoll(argv[i + 1]))) return 1;
    return 0;
  }
  if (argc == 2 && !std::strcmp(argv[1], "identity")) return identity();
  if (argc == 4 && !std::strcmp(argv[1], "offset")) return offset(std::atoll(argv[2]), std::atoll(argv[3]));
  std::fprintf(stderr, "usage: bn_plan_walk cover P C [P C ...] | identity | offset P C\n");
  return 2;
}
