// S2ANet training loss (models/head.py:353-646, utils/loss.py:31-58, models/boxes.py:166-221) on the GPU.
//
// Forward = two launches, no host synchronisation, no floating-point atomics:
//   k_loss_main   one thread per (module, image, anchor of the concatenated levels).  It walks the C class planes of its
//                 level (loads coalesce along W), evaluates the focal BCE of every class and, for a positive anchor, the
//                 relative rbox encode + smooth-L1 of the 5 regression components.  The gradient of the unnormalised,
//                 FPN-weighted loss goes to f32 scratch maps of the prediction shapes (0 for ignored anchors and for the
//                 regression of non-positives); per-workgroup sums (cls, reg, positives) go to the workspace.
//   k_loss_reduce one workgroup: sums the partials in a fixed order (double), applies max(npos, B) and the balances,
//                 writes loss[1], items[4] and the four gradient normalisers.
// Backward = one launch (k_loss_backward): every scratch map times grad_loss[0] * normaliser, in the map's own dtype.
#include "common.hpp"

#include <cmath>

namespace s2a {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxMaps = 4 * S2A_LOSS_MAX_LEVELS;

struct MainArgs {
  s2a_loss_params p;
  int64_t level_start[S2A_LOSS_MAX_LEVELS + 1];   // first anchor of each level in the per-image concatenation
};

__device__ __forceinline__ float ld(const void* p, int dtype, int64_t i) {
  return dtype == S2A_DTYPE_F16 ? (float)static_cast<const _Float16*>(p)[i] : static_cast<const float*>(p)[i];
}

// torch.remainder(a, pi) for f32 (sign of the divisor), then the utils/general.py:925-929 shift
__device__ __forceinline__ float norm_angle(float a) {
  const float lo = -0.785398163397448309616f, pi = 3.14159265358979323846f;
  float r = fmodf(a - lo, pi);
  if (r != 0.0f && r < 0.0f) r += pi;
  return r + lo;
}

__device__ __forceinline__ void block_sum3(double v[3], double* sh) {
  const int t = threadIdx.x;
  for (int k = 0; k < 3; k++) sh[k * kThreads + t] = v[k];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 3; k++) sh[k * kThreads + t] += sh[k * kThreads + t + s];
    __syncthreads();
  }
  for (int k = 0; k < 3; k++) v[k] = sh[k * kThreads];
}

__global__ __launch_bounds__(kThreads) void k_loss_main(MainArgs a, const int64_t* __restrict__ ids,
                                                        const float* __restrict__ targets,
                                                        const int64_t* __restrict__ toff, int64_t A,
                                                        double* __restrict__ partial) {
  __shared__ double sh[3 * kThreads];
  const s2a_loss_params& p = a.p;
  const int B = p.batch, C = p.num_classes;
  const int m = blockIdx.y / B, b = blockIdx.y % B;
  const int64_t ai = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  if (ai < A) {
    int l = 0;
    while (l + 1 < p.n_levels && ai >= a.level_start[l + 1]) l++;
    const s2a_loss_map& mp = p.map[m][l];
    const int64_t HW = (int64_t)mp.height * mp.width, pos = ai - a.level_start[l];
    const float fpn = mp.fpn_balance;
    int64_t id = ids[((int64_t)m * B + b) * A + ai];
    const int64_t ngt = toff[b + 1] - toff[b];
    if (id >= ngt) id = -2;                 // out-of-range assignment: treated as ignored (never read past targets)
    const float* gt = id >= 0 ? targets + (toff[b] + id) * 7 : nullptr;
    int cls_id = -1;
    if (gt) {
      cls_id = (int)gt[1];
      if (cls_id < 0 || cls_id >= C) cls_id = -1;
    }
    // ---- classification: focal BCE with logits over the C planes
    const int64_t cbase = (int64_t)b * C * HW + pos;
    const float alpha = p.fl_alpha, gamma = p.fl_gamma;
    float cls_sum = 0.0f;
    for (int c = 0; c < C; c++) {
      const int64_t i = cbase + c * HW;
      float g = 0.0f;
      if (id != -2) {
        const float x = ld(mp.cls, mp.cls_dtype, i);
        const bool t = c == cls_id;
        const float e = expf(-fabsf(x));
        const float r = 1.0f / (1.0f + e);              // sigmoid(|x|), no overflow for |x| >> 1
        const float ps = x >= 0.0f ? r : e * r;         // sigmoid(x)
        const float qs = x >= 0.0f ? e * r : r;         // 1 - sigmoid(x)
        const float bce = fmaxf(x, 0.0f) - (t ? x : 0.0f) + log1pf(e);
        const float base = t ? qs : ps;                 // 1 - p_t
        const float af = t ? alpha : 1.0f - alpha;
        const float mod = powf(base, gamma);
        // torch's pow backward: exponent * base^(exponent - 1), 0 for exponent 0
        const float dmod = gamma == 0.0f ? 0.0f : gamma * powf(base, gamma - 1.0f) * (t ? -ps * qs : ps * qs);
        cls_sum += af * bce * mod;
        g = af * ((ps - (t ? 1.0f : 0.0f)) * mod + bce * dmod) * fpn;
      }
      mp.grad_cls[i] = g;
    }
    acc[0] = (double)fpn * (double)cls_sum;
    // ---- regression: positives only
    const int64_t bbase = (int64_t)b * 5 * HW + pos;
    if (gt) {
      const float* an = mp.anchors + (int64_t)b * mp.anchor_batch_stride + pos * 5;
      const float ax = an[0], ay = an[1], aw = an[2], ah = an[3], aa = an[4];
      const float ox = gt[2] - ax, oy = gt[3] - ay;
      const float ca = cosf(aa), sa = sinf(aa);
      float tgt[5];
      tgt[0] = (ca * ox + sa * oy) / aw;
      tgt[1] = (-sa * ox + ca * oy) / ah;
      tgt[2] = logf(gt[4] / aw);
      tgt[3] = logf(gt[5] / ah);
      tgt[4] = norm_angle(gt[6] - aa) / 3.14159265358979323846f;
      const float beta = p.smooth_l1_beta;
      float reg_sum = 0.0f;
      for (int k = 0; k < 5; k++) {
        const int64_t i = bbase + k * HW;
        const float d = ld(mp.bbox, mp.bbox_dtype, i) - tgt[k];
        const float ad = fabsf(d);
        float gk;
        if (ad < beta) {
          reg_sum += 0.5f * ad * ad / beta;
          gk = d / beta;
        } else {
          reg_sum += ad - 0.5f * beta;
          gk = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
          // a non-finite delta gives a NaN gradient, as autograd of the reference's where(d < beta, ..) form does
          // (0 * inf from the branch not taken): the overflow must reach the update's found_inf
          if (!(ad <= 3.402823466e+38f)) gk = __builtin_nanf("");
        }
        mp.grad_bbox[i] = gk * fpn;
      }
      acc[1] = (double)fpn * (double)reg_sum;
      acc[2] = 1.0;
    } else {
      for (int k = 0; k < 5; k++) mp.grad_bbox[bbase + k * HW] = 0.0f;
    }
  }
  block_sum3(acc, sh);
  if (threadIdx.x == 0) {
    double* o = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
  }
}

// one workgroup; partial[(m * B + b) * nbx + bx][3]
__global__ __launch_bounds__(kThreads) void k_loss_reduce(const double* __restrict__ partial, int64_t per_module, int B,
                                                          float reg_balance, float odm_balance, float* __restrict__ loss,
                                                          float* __restrict__ items, float* __restrict__ norm) {
  __shared__ double sh[3 * kThreads];
  double tot[2][3];
  for (int m = 0; m < 2; m++) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < per_module; i += kThreads)
      for (int k = 0; k < 3; k++) acc[k] += partial[(m * per_module + i) * 3 + k];
    block_sum3(acc, sh);
    __syncthreads();
    for (int k = 0; k < 3; k++) tot[m][k] = acc[k];
  }
  if (threadIdx.x == 0) {
    const double n0 = fmax(tot[0][2], (double)B), n1 = fmax(tot[1][2], (double)B);
    const float it[4] = {(float)(tot[0][0] / n0), (float)(tot[0][1] / n0 * reg_balance),
                         (float)(tot[1][0] / n1 * odm_balance), (float)(tot[1][1] / n1 * reg_balance * odm_balance)};
    for (int k = 0; k < 4; k++) items[k] = it[k];
    loss[0] = ((it[0] + it[1]) + it[2]) + it[3];
    norm[0] = (float)(1.0 / n0);
    norm[1] = (float)(reg_balance / n0);
    norm[2] = (float)(odm_balance / n1);
    norm[3] = (float)((double)reg_balance * odm_balance / n1);
  }
}

struct BwdArgs {
  s2a_loss_grad_map map[kMaxMaps];
  int64_t blk_start[kMaxMaps + 1];
  int n_maps;
};

constexpr int kBwdPerThread = 4;

__global__ __launch_bounds__(kThreads) void k_loss_backward(BwdArgs a, const float* __restrict__ grad_loss,
                                                            const float* __restrict__ norm) {
  const int64_t blk = blockIdx.x;
  int j = 0;
  while (j + 1 < a.n_maps && blk >= a.blk_start[j + 1]) j++;
  const s2a_loss_grad_map& mp = a.map[j];
  const float s = grad_loss[0] * norm[mp.norm_index];
  const int64_t base = (blk - a.blk_start[j]) * (kThreads * kBwdPerThread) + threadIdx.x;
  for (int k = 0; k < kBwdPerThread; k++) {
    const int64_t i = base + k * kThreads;
    if (i < mp.numel) {
      const float v = mp.src[i] * s;
      if (mp.dtype == S2A_DTYPE_F16)
        static_cast<_Float16*>(mp.dst)[i] = (_Float16)v;
      else
        static_cast<float*>(mp.dst)[i] = v;
    }
  }
}

int64_t blocks_x(int64_t anchors_per_image) { return (anchors_per_image + kThreads - 1) / kThreads; }

}  // namespace
}  // namespace s2a

using namespace s2a;

extern "C" size_t s2a_s2anet_loss_workspace_bytes(int64_t batch, int64_t anchors_per_image) {
  if (batch <= 0 || anchors_per_image <= 0) return 0;
  return align_up((size_t)(2 * batch * blocks_x(anchors_per_image)) * 3 * sizeof(double));
}

extern "C" int s2a_s2anet_loss_forward(const s2a_loss_params* params, const int64_t* assign_ids, const float* targets,
                                       const int64_t* target_offsets, float* loss, float* items, float* norm,
                                       void* workspace, size_t workspace_bytes, s2a_stream_t stream) {
  S2A_CHECK_ARG(params, "s2anet_loss: NULL params");
  const s2a_loss_params& p = *params;
  S2A_CHECK_ARG(p.batch > 0 && p.batch <= 65535 / 2, "s2anet_loss: batch %d out of range", (int)p.batch);
  S2A_CHECK_ARG(p.num_classes > 0, "s2anet_loss: num_classes");
  S2A_CHECK_ARG(p.n_levels > 0 && p.n_levels <= S2A_LOSS_MAX_LEVELS, "s2anet_loss: n_levels %d", (int)p.n_levels);
  S2A_CHECK_ARG(p.smooth_l1_beta > 0.0f, "s2anet_loss: smooth_l1_beta must be > 0");
  MainArgs a{};
  a.p = p;
  a.level_start[0] = 0;
  for (int l = 0; l < p.n_levels; l++) {
    const s2a_loss_map& f = p.map[0][l];
    for (int m = 0; m < 2; m++) {
      const s2a_loss_map& q = p.map[m][l];
      S2A_CHECK_ARG(q.cls && q.bbox && q.anchors && q.grad_cls && q.grad_bbox, "s2anet_loss: NULL map (module %d level %d)", m, l);
      S2A_CHECK_ARG(q.height == f.height && q.width == f.width && q.height > 0 && q.width > 0,
                    "s2anet_loss: level %d sizes differ between the modules", l);
      S2A_CHECK_ARG((q.cls_dtype == S2A_DTYPE_F32 || q.cls_dtype == S2A_DTYPE_F16) &&
                    (q.bbox_dtype == S2A_DTYPE_F32 || q.bbox_dtype == S2A_DTYPE_F16), "s2anet_loss: dtype");
      S2A_CHECK_ARG(q.anchor_batch_stride == 0 || q.anchor_batch_stride == (int64_t)q.height * q.width * 5,
                    "s2anet_loss: anchor_batch_stride must be 0 or H*W*5");
    }
    a.level_start[l + 1] = a.level_start[l] + (int64_t)f.height * f.width;
  }
  const int64_t A = a.level_start[p.n_levels];
  S2A_CHECK_ARG(assign_ids && target_offsets && loss && items && norm, "s2anet_loss: NULL tensor");
  S2A_CHECK_WORKSPACE(workspace, workspace_bytes, s2a_s2anet_loss_workspace_bytes(p.batch, A), "s2anet_loss_forward");
  hipStream_t st = as_stream(stream);
  const int64_t nbx = blocks_x(A);
  double* partial = static_cast<double*>(workspace);
  k_loss_main<<<dim3((unsigned)nbx, (unsigned)(2 * p.batch)), kThreads, 0, st>>>(a, assign_ids, targets, target_offsets, A,
                                                                                 partial);
  S2A_LAUNCH_CHECK();
  k_loss_reduce<<<1, kThreads, 0, st>>>(partial, p.batch * nbx, p.batch, p.reg_balance, p.odm_balance, loss, items, norm);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}

extern "C" int s2a_s2anet_loss_backward(const s2a_loss_grad_map* maps, int n_maps, const float* grad_loss,
                                        const float* norm, s2a_stream_t stream) {
  S2A_CHECK_ARG(maps && n_maps > 0 && n_maps <= kMaxMaps, "s2anet_loss_backward: 1..%d maps", kMaxMaps);
  S2A_CHECK_ARG(grad_loss && norm, "s2anet_loss_backward: NULL tensor");
  BwdArgs a{};
  a.n_maps = n_maps;
  a.blk_start[0] = 0;
  for (int j = 0; j < n_maps; j++) {
    const s2a_loss_grad_map& q = maps[j];
    S2A_CHECK_ARG(q.numel >= 0 && (q.numel == 0 || (q.src && q.dst)), "s2anet_loss_backward: map %d", j);
    S2A_CHECK_ARG(q.dtype == S2A_DTYPE_F32 || q.dtype == S2A_DTYPE_F16, "s2anet_loss_backward: dtype of map %d", j);
    S2A_CHECK_ARG(q.norm_index >= 0 && q.norm_index < 4, "s2anet_loss_backward: norm_index of map %d", j);
    a.map[j] = q;
    a.blk_start[j + 1] = a.blk_start[j] + (q.numel + kThreads * kBwdPerThread - 1) / (kThreads * kBwdPerThread);
  }
  const int64_t nblk = a.blk_start[n_maps];
  if (nblk == 0) return S2A_OK;
  k_loss_backward<<<(unsigned)nblk, kThreads, 0, as_stream(stream)>>>(a, grad_loss, norm);
  S2A_LAUNCH_CHECK();
  return S2A_OK;
}
