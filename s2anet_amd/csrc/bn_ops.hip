// Training-mode BatchNorm for the unfolded trunk (torch.nn.BatchNorm2d as the reference uses it, models/backbone.py:54-83):
// batch statistics, apply (+ residual, + ReLU), and the two backward passes, on f16 channels-last activations seen as [P, C].
// Every pass is one walk over HBM with 16-byte loads; the walk, the slice plan and the moment merges are bn_plan.hpp.
//   * no float atomics, no memset node, no host read; grid and slice count follow from (P, C) only -> capturable, and the same
//     bits every run;
//   * lanes, then slices are combined in a fixed order (lanes inside the workgroup through LDS, slices in a finalise launch of
//     sixteen threads per channel, in double).
#include "bn_plan.hpp"
#include "common.hpp"

namespace s2a {
namespace {

using f16x8n = __attribute__((ext_vector_type(8))) _Float16;
using bn::kRowLanes;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool dtype_ok(int d) { return d == S2A_DTYPE_F32 || d == S2A_DTYPE_F16; }

__device__ __forceinline__ f16x8n ld8(const _Float16* p) { return *reinterpret_cast<const f16x8n*>(p); }
__device__ __forceinline__ void st8(_Float16* p, const f16x8n& v) { *reinterpret_cast<f16x8n*>(p) = v; }

// ================================================================= statistics
// partial: f32 [slices][2][C] = per-slice (mean, M2); an empty slice writes zeros (its count, from the plan, is 0)
__global__ __launch_bounds__(256) void k_bn_stats(const _Float16* __restrict__ x, float* __restrict__ partial, bn::Plan pl) {
  __shared__ float s_mean[kRowLanes][bn::kGroup], s_m2[kRowLanes][bn::kGroup];
  const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
  const int group = blockIdx.x, slice = blockIdx.y, C = pl.C;
  int64_t r0, r1;
  bn::slice_rows(pl, slice, r0, r1);
  const _Float16* col = x + group * bn::kGroup + cx * 8;
  bn::LaneAcc acc[8];
#pragma unroll
  for (int j = 0; j < 8; j++) acc[j].start(0.f);
  int64_t r = r0 + ry;
  const int64_t n = bn::lane_rows(r0, r1, ry);
  if (r < r1) {
    const f16x8n v = ld8(col + r * C);
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j].start((float)v[j]);
    r += kRowLanes;
  }
  for (; r + 3 * kRowLanes < r1; r += 4 * kRowLanes) {      // four requests in flight
    const f16x8n v0 = ld8(col + r * C), v1 = ld8(col + (r + kRowLanes) * C), v2 = ld8(col + (r + 2 * kRowLanes) * C),
                 v3 = ld8(col + (r + 3 * kRowLanes) * C);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      acc[j].add((float)v0[j]);
      acc[j].add((float)v1[j]);
      acc[j].add((float)v2[j]);
      acc[j].add((float)v3[j]);
    }
  }
  for (; r < r1; r += kRowLanes) {
    const f16x8n v = ld8(col + r * C);
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j].add((float)v[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float m = 0.f, q = 0.f;
    if (n > 0) acc[j].finish(n, m, q);
    s_mean[ry][cx * 8 + j] = m;
    s_m2[ry][cx * 8 + j] = q;
  }
  __syncthreads();
  if (tid < bn::kGroup) {
    double m, q;
    bn::merge_moments(&s_mean[0][tid], &s_m2[0][tid], bn::kGroup, 0, 1, kRowLanes, bn::LaneCounts{r0, r1}, m, q);
    const int64_t at = (int64_t)slice * 2 * C + group * bn::kGroup + tid;
    partial[at] = (float)m;
    partial[at + C] = (float)q;
  }
}

// a workgroup of 256 = kFinalChannels channels x kFinalLanes slice lanes (C % 64 == 0: every channel exists)
constexpr int kFinalChannels = 16;
static_assert(kFinalChannels * bn::kFinalLanes == 256, "the finalise launches use 256 threads");

template <typename TR>
__global__ __launch_bounds__(256) void k_bn_stats_final(const float* __restrict__ partial, bn::Plan pl, double eps,
                                                        double momentum, float* __restrict__ mean, float* __restrict__ invstd,
                                                        TR* __restrict__ running_mean, TR* __restrict__ running_var) {
  __shared__ double s_mean[bn::kFinalLanes][kFinalChannels], s_m2[bn::kFinalLanes][kFinalChannels];
  __shared__ int64_t s_n[bn::kFinalLanes][kFinalChannels];
  const int cl = threadIdx.x % kFinalChannels, lane = threadIdx.x / kFinalChannels;
  const int c = blockIdx.x * kFinalChannels + cl;
  double m, q;
  s_n[lane][cl] = bn::final_lane(pl, partial, c, lane, m, q);
  s_mean[lane][cl] = m;
  s_m2[lane][cl] = q;
  __syncthreads();
  if (lane != 0) return;
  bn::final_all(&s_mean[0][cl], &s_m2[0][cl], &s_n[0][cl], kFinalChannels, m, q);
  const double var = q / (double)pl.P;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + eps));
  if (running_mean) running_mean[c] = (TR)(float)((1.0 - momentum) * (double)(float)running_mean[c] + momentum * m);
  if (running_var) {
    const double unbiased = q / (double)(pl.P - 1);
    running_var[c] = (TR)(float)((1.0 - momentum) * (double)(float)running_var[c] + momentum * unbiased);
  }
}

// ================================================================= apply
// out = relu?((x - mean) invstd gamma + beta (+ residual)), f32 throughout, one rounding.  The ReLU is a select that keeps a
// NaN (torch's), not the packed max, which answers 0
template <typename TP>
__global__ __launch_bounds__(256) void k_bn_apply(const _Float16* __restrict__ x, const float* __restrict__ mean,
                                                  const float* __restrict__ invstd, const TP* __restrict__ weight,
                                                  const TP* __restrict__ bias, const _Float16* __restrict__ residual,
                                                  _Float16* __restrict__ out, bn::Plan pl, int relu) {
  const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
  const int c0 = blockIdx.x * bn::kGroup + cx * 8, C = pl.C;
  int64_t r0, r1;
  bn::slice_rows(pl, blockIdx.y, r0, r1);
  if (r0 + ry >= r1) return;
  float mu[8], a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mu[j] = mean[c0 + j];
    a[j] = invstd[c0 + j] * (float)weight[c0 + j];
    b[j] = (float)bias[c0 + j];
  }
#pragma unroll 4
  for (int64_t r = r0 + ry; r < r1; r += kRowLanes) {
    const int64_t at = r * C + c0;
    const f16x8n v = ld8(x + at);
    f16x8n res;
    if (residual) res = ld8(residual + at);
    f16x8n o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float y = ((float)v[j] - mu[j]) * a[j] + b[j];
      if (residual) y += (float)res[j];
      if (relu) y = y < 0.f ? 0.f : y;
      o[j] = (_Float16)y;
    }
    st8(out + at, o);
  }
}

// ================================================================= backward: reduce
// g = out <= 0 ? 0 : grad_out when out is given (the rule of k_conv_bwd_prep: selected, a NaN output passes the gradient);
// partial f32 [slices][2][C] = per-slice (sum g, sum g xhat), xhat = (x - mean) invstd.  g_out, when given, receives g.
// partial == nullptr: the mask alone (g_out wanted, no sums)
__global__ __launch_bounds__(256) void k_bn_bwd_reduce(const _Float16* __restrict__ go, const _Float16* __restrict__ x,
                                                       const _Float16* __restrict__ out, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, _Float16* __restrict__ g_out,
                                                       float* __restrict__ partial, bn::Plan pl) {
  __shared__ float s_g[kRowLanes][bn::kGroup], s_gx[kRowLanes][bn::kGroup];
  const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
  const int c0 = blockIdx.x * bn::kGroup + cx * 8, C = pl.C;
  int64_t r0, r1;
  bn::slice_rows(pl, blockIdx.y, r0, r1);
  float mu[8], is[8], sg[8], sgx[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mu[j] = 0.f;
    is[j] = 0.f;
    sg[j] = 0.f;
    sgx[j] = 0.f;
  }
  if (partial) {                                           // (the mask alone comes without x, mean and invstd: NULL)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      mu[j] = mean[c0 + j];
      is[j] = invstd[c0 + j];
    }
  }
#pragma unroll 4
  for (int64_t r = r0 + ry; r < r1; r += kRowLanes) {
    const int64_t at = r * C + c0;
    f16x8n v = ld8(go + at);
    if (out) {
      const f16x8n y = ld8(out + at);
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (y[j] <= (_Float16)0.f) v[j] = (_Float16)0.f;
      if (g_out) st8(g_out + at, v);
    }
    if (partial) {
      const f16x8n xv = ld8(x + at);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float gv = (float)v[j];
        sg[j] += gv;
        sgx[j] += gv * (((float)xv[j] - mu[j]) * is[j]);
      }
    }
  }
  if (!partial) return;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s_g[ry][cx * 8 + j] = sg[j];
    s_gx[ry][cx * 8 + j] = sgx[j];
  }
  __syncthreads();
  if (tid < bn::kGroup) {
    float a = 0.f, b = 0.f;
    for (int q = 0; q < kRowLanes; q++) {
      a += s_g[q][tid];
      b += s_gx[q][tid];
    }
    const int64_t at = (int64_t)blockIdx.y * 2 * C + blockIdx.x * bn::kGroup + tid;
    partial[at] = a;
    partial[at + C] = b;
  }
}

// slices in slice order -> grad_beta = sum g, grad_gamma = sum g xhat (the parameters' dtype, one rounding), and the two
// coefficients of the input gradient: coef[c] = sum g / P, coef[C + c] = sum g xhat / P
// (the layout of k_bn_stats_final: a thread adds every sixteenth slice in slice order, the sixteen are added in thread order)
template <typename TP>
__global__ __launch_bounds__(256) void k_bn_bwd_final(const float* __restrict__ partial, int slices, int C, int64_t P,
                                                      TP* __restrict__ grad_weight, TP* __restrict__ grad_bias,
                                                      float* __restrict__ coef) {
  __shared__ double s_a[bn::kFinalLanes][kFinalChannels], s_b[bn::kFinalLanes][kFinalChannels];
  const int cl = threadIdx.x % kFinalChannels, lane = threadIdx.x / kFinalChannels;
  const int c = blockIdx.x * kFinalChannels + cl;
  double a = 0.0, b = 0.0;
#pragma unroll 8
  for (int s = lane; s < slices; s += bn::kFinalLanes) {
    a += (double)partial[(int64_t)s * 2 * C + c];
    b += (double)partial[(int64_t)s * 2 * C + C + c];
  }
  s_a[lane][cl] = a;
  s_b[lane][cl] = b;
  __syncthreads();
  if (lane != 0) return;
  a = 0.0;
  b = 0.0;
  for (int q = 0; q < bn::kFinalLanes; q++) {
    a += s_a[q][cl];
    b += s_b[q][cl];
  }
  if (grad_bias) grad_bias[c] = (TP)(float)a;
  if (grad_weight) grad_weight[c] = (TP)(float)b;
  coef[c] = (float)(a / (double)P);
  coef[C + c] = (float)(b / (double)P);
}

// ================================================================= backward: input
// dx = gamma invstd (g - sum g / P - xhat sum g xhat / P); with out given, g is grad_out behind the mask, re-applied here
template <typename TP>
__global__ __launch_bounds__(256) void k_bn_bwd_input(const _Float16* __restrict__ go, const _Float16* __restrict__ x,
                                                      const _Float16* __restrict__ out, const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, const TP* __restrict__ weight,
                                                      const float* __restrict__ coef, _Float16* __restrict__ gx, bn::Plan pl) {
  const int tid = threadIdx.x, cx = tid & 7, ry = tid >> 3;
  const int c0 = blockIdx.x * bn::kGroup + cx * 8, C = pl.C;
  int64_t r0, r1;
  bn::slice_rows(pl, blockIdx.y, r0, r1);
  if (r0 + ry >= r1) return;
  float mu[8], is[8], a[8], k1[8], k2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mu[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
    a[j] = is[j] * (float)weight[c0 + j];
    k1[j] = coef[c0 + j];
    k2[j] = coef[C + c0 + j];
  }
#pragma unroll 4
  for (int64_t r = r0 + ry; r < r1; r += kRowLanes) {
    const int64_t at = r * C + c0;
    f16x8n v = ld8(go + at);
    const f16x8n xv = ld8(x + at);
    if (out) {
      const f16x8n y = ld8(out + at);
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (y[j] <= (_Float16)0.f) v[j] = (_Float16)0.f;
    }
    f16x8n o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float xh = ((float)xv[j] - mu[j]) * is[j];
      o[j] = (_Float16)(a[j] * ((float)v[j] - k1[j] - xh * k2[j]));
    }
    st8(gx + at, o);
  }
}

inline dim3 bn_grid(const bn::Plan& pl) { return dim3((unsigned)pl.groups, (unsigned)pl.slices); }

const char* bn_shape_problem(int64_t P, int64_t C) {
  if (C <= 0 || C % bn::kGroup != 0) return "channels must be a positive multiple of 64";
  if (P < 2) return "training-mode statistics need at least 2 positions";
  if (!bn::plan_ok(P, C)) return "tensor too large for 32-bit offsets (2^31 bytes or more)";
  return nullptr;
}

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" int s2a_bn_slices(int64_t positions, int64_t channels) { return bn::plan_slices(positions, channels); }

extern "C" int s2a_bn_train_stats_f16(const void* x, int64_t positions, int64_t channels, double eps, double momentum,
                                      float* partial, int slices, float* mean, float* invstd, void* running_mean,
                                      void* running_var, int running_dtype, s2a_stream_t stream) {
  const char* problem = bn_shape_problem(positions, channels);
  S2A_CHECK_ARG(!problem, "bn_train_stats: %s", problem);
  S2A_CHECK_ARG(eps >= 0.0 && momentum >= 0.0 && momentum <= 1.0, "bn_train_stats: eps must be >= 0 and momentum in [0, 1]");
  const int want = bn::plan_slices(positions, channels);
  S2A_CHECK_ARG(slices == want, "bn_train_stats: slices is %d, s2a_bn_slices answers %d", slices, want);
  S2A_CHECK_ARG(x && partial && mean && invstd, "bn_train_stats: NULL tensor");
  S2A_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn_train_stats: running_mean and running_var go together");
  S2A_CHECK_ARG(!running_mean || dtype_ok(running_dtype), "bn_train_stats: running statistics must be f32 or f16");
  S2A_CHECK_ARG(aligned16(x) && aligned16(partial) && aligned4(mean) && aligned4(invstd) && aligned4(running_mean) &&
                    aligned4(running_var),
                "bn_train_stats: tensors must be aligned (x and partial to 16 bytes, the vectors to 4)");
  const bn::Plan pl = bn::make_plan(positions, channels);
  hipStream_t st = as_stream(stream);
  k_bn_stats<<<bn_grid(pl), 256, 0, st>>>((const _Float16*)x, partial, pl);
  S2A_LAUNCH_CHECK();
  const unsigned fb = (unsigned)(channels / kFinalChannels);
  if (running_mean && running_dtype == S2A_DTYPE_F16)
    k_bn_stats_final<_Float16><<<fb, 256, 0, st>>>(partial, pl, eps, momentum, mean, invstd, (_Float16*)running_mean,
                                                  (_Float16*)running_var);
  else
    k_bn_stats_final<float><<<fb, 256, 0, st>>>(partial, pl, eps, momentum, mean, invstd, (float*)running_mean, (float*)running_var);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_bn_train_apply_f16(const void* x, const float* mean, const float* invstd, const void* weight, const void* bias,
                                      int param_dtype, const void* residual, void* out, int64_t positions, int64_t channels,
                                      int relu, s2a_stream_t stream) {
  const char* problem = bn_shape_problem(positions, channels);
  S2A_CHECK_ARG(!problem, "bn_train_apply: %s", problem);
  S2A_CHECK_ARG(dtype_ok(param_dtype), "bn_train_apply: weight / bias dtype must be f32 or f16");
  S2A_CHECK_ARG(x && mean && invstd && weight && bias && out, "bn_train_apply: NULL tensor");
  S2A_CHECK_ARG(aligned16(x) && aligned16(residual) && aligned16(out) && aligned4(mean) && aligned4(invstd) && aligned4(weight) &&
                    aligned4(bias),
                "bn_train_apply: tensors must be aligned (activations to 16 bytes, the vectors to 4)");
  const bn::Plan pl = bn::make_plan(positions, channels);
  hipStream_t st = as_stream(stream);
  if (param_dtype == S2A_DTYPE_F32)
    k_bn_apply<float><<<bn_grid(pl), 256, 0, st>>>((const _Float16*)x, mean, invstd, (const float*)weight, (const float*)bias,
                                                   (const _Float16*)residual, (_Float16*)out, pl, relu != 0);
  else
    k_bn_apply<_Float16><<<bn_grid(pl), 256, 0, st>>>((const _Float16*)x, mean, invstd, (const _Float16*)weight,
                                                      (const _Float16*)bias, (const _Float16*)residual, (_Float16*)out, pl,
                                                      relu != 0);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_bn_backward_reduce_f16(const void* grad_out, const void* x, const void* out, const float* mean,
                                          const float* invstd, void* g, float* partial, int slices, void* grad_weight,
                                          void* grad_bias, int param_dtype, float* coef, int64_t positions, int64_t channels,
                                          s2a_stream_t stream) {
  const char* problem = bn_shape_problem(positions, channels);
  S2A_CHECK_ARG(!problem, "bn_backward_reduce: %s", problem);
  S2A_CHECK_ARG(!g || out, "bn_backward_reduce: a masked gradient needs the forward output");
  S2A_CHECK_ARG(partial || g, "bn_backward_reduce: nothing to write (neither partial nor g)");
  S2A_CHECK_ARG(grad_out, "bn_backward_reduce: NULL tensor");
  S2A_CHECK_ARG(aligned16(grad_out) && aligned16(x) && aligned16(out) && aligned16(g) && aligned16(partial),
                "bn_backward_reduce: tensors must be 16-byte aligned");
  if (partial) {
    const int want = bn::plan_slices(positions, channels);
    S2A_CHECK_ARG(slices == want, "bn_backward_reduce: slices is %d, s2a_bn_slices answers %d", slices, want);
    S2A_CHECK_ARG(x && mean && invstd && coef, "bn_backward_reduce: NULL tensor (the sums need x, mean, invstd and coef)");
    S2A_CHECK_ARG((!grad_weight && !grad_bias) || dtype_ok(param_dtype), "bn_backward_reduce: gradient dtype must be f32 or f16");
    S2A_CHECK_ARG(aligned4(mean) && aligned4(invstd) && aligned4(coef) && aligned4(grad_weight) && aligned4(grad_bias),
                  "bn_backward_reduce: the vectors must be 4-byte aligned");
  } else {
    S2A_CHECK_ARG(!grad_weight && !grad_bias && !coef, "bn_backward_reduce: gradients and coefficients need partial");
  }
  const bn::Plan pl = bn::make_plan(positions, channels);
  hipStream_t st = as_stream(stream);
  k_bn_bwd_reduce<<<bn_grid(pl), 256, 0, st>>>((const _Float16*)grad_out, (const _Float16*)x, (const _Float16*)out, mean, invstd,
                                               (_Float16*)g, partial, pl);
  S2A_LAUNCH_CHECK();
  if (partial) {
    const unsigned fb = (unsigned)(channels / kFinalChannels);
    if (param_dtype == S2A_DTYPE_F16 && (grad_weight || grad_bias))
      k_bn_bwd_final<_Float16><<<fb, 256, 0, st>>>(partial, pl.slices, pl.C, pl.P, (_Float16*)grad_weight, (_Float16*)grad_bias, coef);
    else
      k_bn_bwd_final<float><<<fb, 256, 0, st>>>(partial, pl.slices, pl.C, pl.P, (float*)grad_weight, (float*)grad_bias, coef);
    S2A_LAUNCH_CHECK();
  }
  return S2A_OK;
}

extern "C" int s2a_bn_backward_input_f16(const void* g, const void* x, const void* out, const float* mean, const float* invstd,
                                         const void* weight, int param_dtype, const float* coef, void* grad_input,
                                         int64_t positions, int64_t channels, s2a_stream_t stream) {
  const char* problem = bn_shape_problem(positions, channels);
  S2A_CHECK_ARG(!problem, "bn_backward_input: %s", problem);
  S2A_CHECK_ARG(dtype_ok(param_dtype), "bn_backward_input: weight dtype must be f32 or f16");
  S2A_CHECK_ARG(g && x && mean && invstd && weight && coef && grad_input, "bn_backward_input: NULL tensor");
  S2A_CHECK_ARG(aligned16(g) && aligned16(x) && aligned16(out) && aligned16(grad_input) && aligned4(mean) && aligned4(invstd) &&
                    aligned4(weight) && aligned4(coef),
                "bn_backward_input: tensors must be aligned (activations to 16 bytes, the vectors to 4)");
  const bn::Plan pl = bn::make_plan(positions, channels);
  hipStream_t st = as_stream(stream);
  if (param_dtype == S2A_DTYPE_F32)
    k_bn_bwd_input<float><<<bn_grid(pl), 256, 0, st>>>((const _Float16*)g, (const _Float16*)x, (const _Float16*)out, mean, invstd,
                                                       (const float*)weight, coef, (_Float16*)grad_input, pl);
  else
    k_bn_bwd_input<_Float16><<<bn_grid(pl), 256, 0, st>>>((const _Float16*)g, (const _Float16*)x, (const _Float16*)out, mean,
                                                          invstd, (const _Float16*)weight, coef, (_Float16*)grad_input, pl);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
