// Training update (train.py:358-373, utils/torch_utils.py:276-307 of the reference) as three launches: GradScaler.unscale_
// + clip_grad_norm_ + SGD (momentum / Nesterov, parameter groups) + scaler.update + zero_grad + ModelEMA.update.
//
// Multi-tensor: the tensors live in a device table, a device chunk map gives every workgroup (tensor, start), so a
// workgroup never straddles two tensors and no tensor address travels as a kernel argument.
//   k_optim_partials  per trained chunk: f32 sum of (g * inv_scale)^2 and a non-finite flag (per-element test), one pair
//                     per chunk, reduced in a fixed order -> bit-reproducible, no atomics
//   k_optim_finalise  one workgroup: partials in chunk order in double -> norm, clip, found_inf, skip; the GradScaler
//                     state, the EMA decay; the control block of the apply launch and the stats
//   k_optim_apply     per element: the SGD step (unless skipped), the EMA, grad = 0
// Memory-bound: rows whose pointers are all 16-byte aligned use 16-byte accesses, others and tails go element-wise.
#include "common.hpp"

#include <cmath>

namespace s2a {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = S2A_OPTIM_CHUNK;
constexpr int kMaxGrid = 1 << 20;

// what launch 2 hands to launch 3 (workspace)
struct Ctrl {
  float inv_scale, clip, d, one_minus_d;
  int32_t skip_update, pad[3];
};

__device__ __forceinline__ float inv_scale_of(const float* scale, int enabled) {
  // GradScaler.unscale_: scale.double().reciprocal().float()
  return enabled ? (float)(1.0 / (double)scale[0]) : 1.0f;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

__global__ __launch_bounds__(kThreads) void k_optim_partials(const s2a_optim_tensor* __restrict__ tensors,
                                                             const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                             const float* __restrict__ scale, int scaling_enabled,
                                                             float* __restrict__ partial, uint32_t* __restrict__ flags) {
  __shared__ float sh[kThreads];
  __shared__ uint32_t sh_bad[kThreads];
  const int t = threadIdx.x;
  const float inv = inv_scale_of(scale, scaling_enabled);
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const s2a_optim_tensor row = tensors[chunks[2 * c]];
    const int64_t start = chunks[2 * c + 1];
    const int64_t left = row.numel - start;
    const int n = left < kChunk ? (int)left : kChunk;
    const float* g = row.grad + start;
    float acc = 0.0f;
    uint32_t bad = 0;
    int done = 0;
    if (aligned16(g, nullptr, nullptr, nullptr)) {
      const int n4 = n >> 2;
      const float4* g4 = reinterpret_cast<const float4*>(g);
      for (int i = t; i < n4; i += kThreads) {
        const float4 v = g4[i];
        const float a0 = v.x * inv, a1 = v.y * inv, a2 = v.z * inv, a3 = v.w * inv;
        bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
        acc += a0 * a0;
        acc += a1 * a1;
        acc += a2 * a2;
        acc += a3 * a3;
      }
      done = n4 << 2;
    }
    for (int i = done + t; i < n; i += kThreads) {
      const float v = g[i];
      const float a = v * inv;
      bad |= !isfinite(v);
      acc += a * a;
    }
    sh[t] = acc;
    sh_bad[t] = bad;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if (t < s) {
        sh[t] += sh[t + s];
        sh_bad[t] |= sh_bad[t + s];
      }
      __syncthreads();
    }
    if (t == 0) {
      partial[c] = sh[0];
      flags[c] = sh_bad[0];
    }
    __syncthreads();   // sh is reused by the next chunk of this workgroup
  }
}

struct FinaliseArgs {
  const float* partial;
  const uint32_t* flags;
  int64_t n_partials;   // 0: launch 1 was skipped
  float* scale;
  int32_t* counters;
  const void* skip;
  int32_t skip_elem_bytes, scaling_enabled, growth_interval;
  float max_norm, growth, backoff;
  double ema_decay, ema_tau;
  Ctrl* ctrl;
  float* stats;
};

__global__ __launch_bounds__(kThreads) void k_optim_finalise(FinaliseArgs a) {
  __shared__ double sh[kThreads];
  __shared__ uint32_t sh_bad[kThreads];
  const int t = threadIdx.x;
  // fixed order: thread t owns the contiguous run [t * per, (t + 1) * per) of the partials, the runs are then added pairwise
  const int64_t per = (a.n_partials + kThreads - 1) / kThreads;
  const int64_t lo = t * per, hi = lo + per < a.n_partials ? lo + per : a.n_partials;
  double acc = 0.0;
  uint32_t bad = 0;
  for (int64_t i = lo; i < hi; i++) {
    acc += (double)a.partial[i];
    bad |= a.flags[i];
  }
  sh[t] = acc;
  sh_bad[t] = bad;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      sh[t] += sh[t + s];
      sh_bad[t] |= sh_bad[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  const double total = sqrt(sh[0]);
  const int found_inf = sh_bad[0] != 0;
  float clip = 1.0f;
  if (a.max_norm > 0.0f) {
    // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN coefficient stays NaN
    const float c = (float)((double)a.max_norm / (total + 1e-6));
    clip = c < 1.0f ? c : (c != c ? c : 1.0f);
  }
  int skip = a.scaling_enabled && found_inf;
  if (a.skip != nullptr) {
    const long long s = a.skip_elem_bytes == 8 ? *static_cast<const long long*>(a.skip) : (long long)*static_cast<const int*>(a.skip);
    skip |= s != 0;
  }
  float inv = 1.0f, new_scale = 1.0f;
  int tracker = a.counters[0];
  if (a.scaling_enabled) {
    const float sc = a.scale[0];
    inv = (float)(1.0 / (double)sc);
    new_scale = sc;
    if (found_inf) {
      new_scale = sc * a.backoff;
      tracker = 0;
    } else if (tracker + 1 == a.growth_interval) {
      const float grown = sc * a.growth;
      if (isfinite(grown)) new_scale = grown;
      tracker = 0;
    } else {
      tracker = tracker + 1;
    }
    a.scale[0] = new_scale;
    a.counters[0] = tracker;
  }
  const int updates = a.counters[1] + 1;
  a.counters[1] = updates;
  const double d = a.ema_decay * (1.0 - exp(-(double)updates / a.ema_tau));
  Ctrl c;
  c.inv_scale = inv;
  c.clip = clip;
  c.d = (float)d;
  c.one_minus_d = (float)(1.0 - d);
  c.skip_update = skip;
  c.pad[0] = c.pad[1] = c.pad[2] = 0;
  *a.ctrl = c;
  a.stats[0] = (float)total;
  a.stats[1] = clip;
  a.stats[2] = (float)found_inf;
  a.stats[3] = (float)skip;
  a.stats[4] = new_scale;
  a.stats[5] = (float)d;
  a.stats[6] = (float)updates;
  a.stats[7] = (float)tracker;
}

struct Hyper {
  float lr, momentum, wd;
  bool nesterov;
};

// one element of a trained tensor that is not skipped: new p, new buf
__device__ __forceinline__ void sgd(float& p, float& buf, float grad, float inv, float clip, const Hyper& h) {
  float g = grad * inv;
  g = g * clip;
  if (h.wd != 0.0f) g = g + h.wd * p;
  buf = h.momentum * buf + g;
  g = h.nesterov ? g + h.momentum * buf : buf;
  p = p - h.lr * g;
}

__global__ __launch_bounds__(kThreads) void k_optim_apply(const s2a_optim_tensor* __restrict__ tensors,
                                                          const int64_t* __restrict__ chunks, int64_t n_chunks,
                                                          const float* __restrict__ lr, const float* __restrict__ hyper,
                                                          const Ctrl* __restrict__ ctrl_p) {
  const int t = threadIdx.x;
  const Ctrl ctrl = *ctrl_p;
  const float d = ctrl.d, omd = ctrl.one_minus_d;
  const bool update = ctrl.skip_update == 0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const s2a_optim_tensor row = tensors[chunks[2 * c]];
    const int64_t start = chunks[2 * c + 1];
    const int64_t left = row.numel - start;
    const int n = left < kChunk ? (int)left : kChunk;
    float* p = row.p + start;
    float* e = row.ema ? row.ema + start : nullptr;
    if (row.kind == S2A_OPTIM_EMA_ONLY) {
      if (e == nullptr) continue;
      int done = 0;
      if (aligned16(p, e, nullptr, nullptr)) {
        const int n4 = n >> 2;
        const float4* p4 = reinterpret_cast<const float4*>(p);
        float4* e4 = reinterpret_cast<float4*>(e);
        for (int i = t; i < n4; i += kThreads) {
          const float4 pv = p4[i];
          float4 ev = e4[i];
          ev.x = d * ev.x + omd * pv.x;
          ev.y = d * ev.y + omd * pv.y;
          ev.z = d * ev.z + omd * pv.z;
          ev.w = d * ev.w + omd * pv.w;
          e4[i] = ev;
        }
        done = n4 << 2;
      }
      for (int i = done + t; i < n; i += kThreads) e[i] = d * e[i] + omd * p[i];
      continue;
    }
    float* g = row.grad + start;
    float* b = row.momentum_buf + start;
    Hyper h;
    h.lr = lr[row.group];
    h.momentum = hyper[4 * row.group + 0];
    h.wd = hyper[4 * row.group + 1];
    h.nesterov = hyper[4 * row.group + 2] != 0.0f;
    int done = 0;
    if (aligned16(p, g, b, e)) {
      const int n4 = n >> 2;
      float4* p4 = reinterpret_cast<float4*>(p);
      float4* g4 = reinterpret_cast<float4*>(g);
      float4* b4 = reinterpret_cast<float4*>(b);
      float4* e4 = reinterpret_cast<float4*>(e);
      for (int i = t; i < n4; i += kThreads) {
        float4 pv = p4[i];
        if (update) {
          const float4 gv = g4[i];
          float4 bv = b4[i];
          sgd(pv.x, bv.x, gv.x, ctrl.inv_scale, ctrl.clip, h);
          sgd(pv.y, bv.y, gv.y, ctrl.inv_scale, ctrl.clip, h);
          sgd(pv.z, bv.z, gv.z, ctrl.inv_scale, ctrl.clip, h);
          sgd(pv.w, bv.w, gv.w, ctrl.inv_scale, ctrl.clip, h);
          p4[i] = pv;
          b4[i] = bv;
        }
        if (e != nullptr) {
          float4 ev = e4[i];
          ev.x = d * ev.x + omd * pv.x;
          ev.y = d * ev.y + omd * pv.y;
          ev.z = d * ev.z + omd * pv.z;
          ev.w = d * ev.w + omd * pv.w;
          e4[i] = ev;
        }
        g4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
      done = n4 << 2;
    }
    for (int i = done + t; i < n; i += kThreads) {
      float pv = p[i];
      if (update) {
        float bv = b[i];
        sgd(pv, bv, g[i], ctrl.inv_scale, ctrl.clip, h);
        p[i] = pv;
        b[i] = bv;
      }
      if (e != nullptr) e[i] = d * e[i] + omd * pv;
      g[i] = 0.0f;
    }
  }
}

struct UpdateWs { Ctrl* ctrl; float* partial; uint32_t* flags; };   // carved from the workspace, in this order
bool carve(Carver& cv, int64_t n_trained_chunks, UpdateWs& w) {
  w.ctrl = cv.take<Ctrl>(1);
  w.partial = cv.take<float>((size_t)n_trained_chunks);
  w.flags = cv.take<uint32_t>((size_t)n_trained_chunks);
  return cv.ok();
}
constexpr size_t kUpdateWsSlack = 0;   // none: the query is exactly the carve

}  // namespace
}  // namespace s2a

extern "C" size_t s2a_train_update_workspace_bytes(int64_t n_trained_chunks) {
  if (n_trained_chunks < 0) return 0;
  return s2a::carved_bytes<s2a::UpdateWs>(n_trained_chunks) + s2a::kUpdateWsSlack;
}

extern "C" int s2a_train_update(const s2a_train_update_args* args, void* workspace, size_t workspace_bytes,
                                s2a_stream_t stream) {
  using namespace s2a;
  S2A_CHECK_ARG(args != nullptr, "s2a_train_update: NULL args");
  const s2a_train_update_args& a = *args;
  S2A_CHECK_ARG(a.n_tensors >= 0 && a.n_chunks >= 0 && a.n_trained_chunks >= 0 && a.n_trained_chunks <= a.n_chunks,
                "s2a_train_update: bad counts (tensors %lld, chunks %lld, trained chunks %lld)", (long long)a.n_tensors,
                (long long)a.n_chunks, (long long)a.n_trained_chunks);
  S2A_CHECK_ARG(a.n_chunks == 0 || (a.tensors != nullptr && a.chunks != nullptr && a.n_tensors > 0),
                "s2a_train_update: NULL tensor table / chunk map");
  S2A_CHECK_ARG(a.n_trained_chunks == 0 || (a.lr != nullptr && a.hyper != nullptr && a.n_groups > 0),
                "s2a_train_update: NULL lr / hyper table");
  S2A_CHECK_ARG(a.counters != nullptr && a.stats != nullptr, "s2a_train_update: NULL counters / stats");
  S2A_CHECK_ARG(!a.scaling_enabled || a.scale != nullptr, "s2a_train_update: scaling enabled with a NULL scale");
  S2A_CHECK_ARG(a.skip == nullptr || a.skip_elem_bytes == 4 || a.skip_elem_bytes == 8,
                "s2a_train_update: skip flag must be int32 or int64 (skip_elem_bytes 4 or 8, got %d)", a.skip_elem_bytes);
  S2A_CHECK_ARG(!a.scaling_enabled || a.growth_interval > 0, "s2a_train_update: growth_interval must be positive");
  S2A_CHECK_ARG(a.ema_tau > 0.0, "s2a_train_update: ema_tau must be positive");
  UpdateWs w;
  if (int rc = carve_workspace(workspace, workspace_bytes, w, kUpdateWsSlack, "s2a_train_update", a.n_trained_chunks)) return rc;
  S2A_CHECK_ARG(((uintptr_t)workspace & 15u) == 0, "s2a_train_update: workspace must be 16-byte aligned");
  hipStream_t st = as_stream(stream);

  const bool need_norm = (a.max_norm > 0.0f || a.scaling_enabled) && a.n_trained_chunks > 0;
  if (need_norm) {
    const int grid = (int)(a.n_trained_chunks < kMaxGrid ? a.n_trained_chunks : kMaxGrid);
    k_optim_partials<<<grid, kThreads, 0, st>>>(a.tensors, a.chunks, a.n_trained_chunks, a.scale, a.scaling_enabled,
                                                 w.partial, w.flags);
    S2A_LAUNCH_CHECK();
  }
  FinaliseArgs f;
  f.partial = w.partial;
  f.flags = w.flags;
  f.n_partials = need_norm ? a.n_trained_chunks : 0;
  f.scale = a.scale;
  f.counters = a.counters;
  f.skip = a.skip;
  f.skip_elem_bytes = a.skip_elem_bytes;
  f.scaling_enabled = a.scaling_enabled;
  f.growth_interval = a.growth_interval;
  f.max_norm = a.max_norm;
  f.growth = a.growth_factor;
  f.backoff = a.backoff_factor;
  f.ema_decay = a.ema_decay;
  f.ema_tau = a.ema_tau;
  f.ctrl = w.ctrl;
  f.stats = a.stats;
  k_optim_finalise<<<1, kThreads, 0, st>>>(f);
  S2A_LAUNCH_CHECK();
  if (a.n_chunks > 0) {
    const int grid = (int)(a.n_chunks < kMaxGrid ? a.n_chunks : kMaxGrid);
    k_optim_apply<<<grid, kThreads, 0, st>>>(a.tensors, a.chunks, a.n_chunks, a.lr, a.hyper, w.ctrl);
    S2A_LAUNCH_CHECK();
  }
  return S2A_OK;
}
