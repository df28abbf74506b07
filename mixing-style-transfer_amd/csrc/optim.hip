// The optimiser tail of both training steps and of the per-pair fit, over an ordered LIST of fp32 tensors per call:
//   mst_optim_grad_norm + mst_optim_scale_grads = torch.nn.utils.clip_grad_norm_ (norm_type 2),
//   mst_optim_step = one step of torch.optim.Adam / AdamW / SGD(momentum) from their single-tensor formulas,
//   mst_keep_best  = the fit loop's `if distance < best_distance` bookkeeping, on the device.
// (src/train_style_transfer.py:284-288, 602-605; src/train.py:292-296, 323-326; inference/test_tcn_style_transfer.py:130-189.)
//
// One workgroup = one (tensor, chunk) of kChunk elements, found through the caller's chunk map; an element's result is a pure
// function of its own inputs and the call's scalars: every update is evaluated in double from the fp32 inputs (contraction off,
// one rounding to fp32 per stored value), by the same device function on the scalar head / tail and on the 16-byte body.  No
// float atomics and no workgroup waits on another: the norm is per-chunk double partials (a fixed tree inside the workgroup)
// that a second single-workgroup launch adds in index order.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kChunk = 4096, kThreads = 256, kWaves = kThreads / 64;
constexpr int kMaxCopies = 8, kCopyBlocks = 256;

struct Chunk {
  mst_optim_tensor t;
  long long start;
  int len;   // <= 0: nothing to do (a map entry past its tensor's end)
};

__device__ __forceinline__ Chunk chunk_of(const mst_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ map) {
  Chunk c;
  const int ti = map[2 * (size_t)blockIdx.x], ci = map[2 * (size_t)blockIdx.x + 1];
  c.t = tensors[ti];
  c.start = (long long)ci * kChunk;
  const long long left = c.t.n - c.start;
  c.len = (int)(left < kChunk ? left : kChunk);
  return c;
}

// elements before the first 16-byte boundary of p (p is 4-byte aligned)
__device__ __forceinline__ int head_of(const void* p) { return (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2); }

// ---- norm ------------------------------------------------------------------------------------------------------------------
// Element j of the chunk goes to thread j % 256 whatever the pointer's alignment (dword loads, coalesced), so a chunk's partial
// depends on its values alone.
__global__ __launch_bounds__(kThreads) void optim_sumsq_kernel(const mst_optim_tensor* __restrict__ tensors,
                                                               const int32_t* __restrict__ map, double* __restrict__ part) {
  __shared__ double red[kWaves];
  const Chunk c = chunk_of(tensors, map);
  const int tid = threadIdx.x;
  double a = 0.0;
  if (c.len > 0) {
    const float* g = c.t.grad + c.start;
#pragma unroll 4
    for (int j = tid; j < c.len; j += kThreads) {
      const double v = (double)g[j];
      a += v * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// norm = fp32(sqrt(sum)), coef = min(1, max_norm * (1 / (norm + 1e-6))) in fp32: clip_grad_norm_'s
// `torch.clamp(max_norm / (total_norm + 1e-6), max=1.0)`, whose scalar / tensor is reciprocal-then-multiply.  NaN stays NaN.
__global__ __launch_bounds__(kThreads) void optim_norm_fold_kernel(const double* __restrict__ part, int n_chunks, float max_norm,
                                                                   float* __restrict__ norm_out, float* __restrict__ coef_out) {
  __shared__ double red[kThreads];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int i = tid; i < n_chunks; i += kThreads) a += part[i];
  red[tid] = a;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const float norm = (float)sqrt(red[0]);
    float coef = max_norm * __fdiv_rn(1.0f, norm + 1e-6f);
    if (coef > 1.0f) coef = 1.0f;   // (false for NaN)
    *norm_out = norm;
    *coef_out = coef;
  }
}

__global__ __launch_bounds__(kThreads) void optim_scale_kernel(const mst_optim_tensor* __restrict__ tensors,
                                                               const int32_t* __restrict__ map, const float* __restrict__ coef_p) {
  const Chunk c = chunk_of(tensors, map);
  if (c.len <= 0) return;
  const float coef = *coef_p;
  float* g = c.t.grad + c.start;
  const int tid = threadIdx.x, head = min(head_of(g), c.len), nvec = (c.len - head) >> 2, tail0 = head + 4 * nvec;
  float4* gv = reinterpret_cast<float4*>(g + head);
  for (int v = tid; v < nvec; v += kThreads) {
    float4 x = gv[v];
    x.x *= coef, x.y *= coef, x.z *= coef, x.w *= coef;
    gv[v] = x;
  }
  if (tid < head) g[tid] *= coef;
  if (tail0 + tid < c.len) g[tail0 + tid] *= coef;
}

// ---- step ------------------------------------------------------------------------------------------------------------------
struct Hyper {
  double lr, beta1, beta2, eps, wd, momentum;
};
struct StepScalars {   // per tensor, from its step count
  double step_size, bc2_sqrt;
};

// Adam / AdamW: step += 1 and the bias corrections of the new count, one thread per tensor.  Skipped whole under found_inf.
__global__ void optim_prep_kernel(const mst_optim_tensor* __restrict__ tensors, int n_tensors, Hyper h,
                                  const float* __restrict__ found_inf, StepScalars* __restrict__ sc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_tensors || (found_inf && *found_inf != 0.f)) return;
  const float t = *tensors[i].step + 1.0f;
  *tensors[i].step = t;
  const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
  sc[i].step_size = h.lr / bc1;
  sc[i].bc2_sqrt = sqrt(bc2);
}

template <int ALGO>
struct Update {
  Hyper h;
  StepScalars s;
  double inv_scale;
  // torch.optim's single-tensor formulas, in double from the fp32 inputs; p, s1, s2 are rounded once each
  __device__ __forceinline__ void operator()(float& p32, float g32, float& s1, float& s2) const {
    double g = (double)g32 * inv_scale, p = (double)p32;
    if (ALGO == MST_OPTIM_SGD) {
      if (h.wd != 0.0) g = g + h.wd * p;
      if (h.momentum != 0.0) {
        g = h.momentum * (double)s1 + g;   // a zero buffer gives g itself: the first step's copy
        s1 = (float)g;
      }
      p32 = (float)(p - h.lr * g);
      return;
    }
    if (ALGO == MST_OPTIM_ADAM && h.wd != 0.0) g = g + h.wd * p;
    if (ALGO == MST_OPTIM_ADAMW) p = p * (1.0 - h.lr * h.wd);
    double m = (double)s1, v = (double)s2;
    m = m + (g - m) * (1.0 - h.beta1);
    v = h.beta2 * v + (1.0 - h.beta2) * g * g;
    const double denom = sqrt(v) / s.bc2_sqrt + h.eps;
    s1 = (float)m, s2 = (float)v;
    p32 = (float)(p - s.step_size * (m / denom));
  }
};

template <int ALGO>
__global__ __launch_bounds__(kThreads) void optim_step_kernel(const mst_optim_tensor* __restrict__ tensors,
                                                              const int32_t* __restrict__ map, Hyper h,
                                                              const StepScalars* __restrict__ sc, const float* __restrict__ grad_scale,
                                                              const float* __restrict__ found_inf) {
  if (found_inf && *found_inf != 0.f) return;
  const Chunk c = chunk_of(tensors, map);
  if (c.len <= 0) return;
  constexpr bool kS2 = ALGO != MST_OPTIM_SGD;   // exp_avg_sq
  Update<ALGO> up;
  up.h = h;
  up.s = ALGO == MST_OPTIM_SGD ? StepScalars{0.0, 1.0} : sc[map[2 * (size_t)blockIdx.x]];
  up.inv_scale = grad_scale ? 1.0 / (double)*grad_scale : 1.0;
  float* p = c.t.param + c.start;
  const float* g = c.t.grad + c.start;
  const bool has1 = c.t.state1 != nullptr;   // (SGD without momentum has no buffer)
  float* s1 = has1 ? c.t.state1 + c.start : nullptr;
  float* s2 = kS2 ? c.t.state2 + c.start : nullptr;
  const int tid = threadIdx.x;
  auto one = [&](int j) {
    float pj = p[j], a = has1 ? s1[j] : 0.f, b = kS2 ? s2[j] : 0.f;
    up(pj, g[j], a, b);
    p[j] = pj;
    if (has1) s1[j] = a;
    if (kS2) s2[j] = b;
  };
  // 16-byte body only when every array of the tensor reaches a 16-byte boundary after the same number of elements
  int head = head_of(p);
  const bool wide = head_of(g) == head && (!has1 || head_of(s1) == head) && (!kS2 || head_of(s2) == head);
  if (!wide) {
    for (int j = tid; j < c.len; j += kThreads) one(j);
    return;
  }
  head = min(head, c.len);
  const int nvec = (c.len - head) >> 2, tail0 = head + 4 * nvec;
  for (int v = tid; v < nvec; v += kThreads) {
    const int j = head + 4 * v;
    float4 pv = *reinterpret_cast<float4*>(p + j);
    const float4 gv = *reinterpret_cast<const float4*>(g + j);
    float4 av = has1 ? *reinterpret_cast<float4*>(s1 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 bv = kS2 ? *reinterpret_cast<float4*>(s2 + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    up(pv.x, gv.x, av.x, bv.x), up(pv.y, gv.y, av.y, bv.y), up(pv.z, gv.z, av.z, bv.z), up(pv.w, gv.w, av.w, bv.w);
    *reinterpret_cast<float4*>(p + j) = pv;
    if (has1) *reinterpret_cast<float4*>(s1 + j) = av;
    if (kS2) *reinterpret_cast<float4*>(s2 + j) = bv;
  }
  if (tid < head) one(tid);
  if (tail0 + tid < c.len) one(tail0 + tid);
}

// ---- keep best -------------------------------------------------------------------------------------------------------------
struct Copies {
  const uint32_t* src[kMaxCopies];
  uint32_t* dst[kMaxCopies];
  long long words[kMaxCopies];
};

// Launch 1 of 2: every workgroup reads the same (loss, best) -- nobody writes them here -- and copies its share when loss < best.
__global__ __launch_bounds__(kThreads) void keep_best_copy_kernel(const float* __restrict__ loss, const float* __restrict__ best,
                                                                  Copies cp) {
  if (!(*loss < *best)) return;   // (false for a NaN loss)
  const int k = blockIdx.y;
  const uint32_t* s = cp.src[k];
  uint32_t* d = cp.dst[k];
  const long long n = cp.words[k], stride = (long long)gridDim.x * kThreads;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) d[i] = s[i];
}

// Launch 2 of 2: the history entry, and the new best with its index.
__global__ void keep_best_update_kernel(const float* __restrict__ loss, float* __restrict__ best, int32_t* __restrict__ best_index,
                                        float* __restrict__ history, int index) {
  const float l = *loss;
  if (history) history[index] = l;
  if (l < *best) {
    *best = l;
    *best_index = index;
  }
}

int list_ok(const mst_optim_list* list, const char* what) {
  MST_REQUIRE(list, "%s: NULL list", what);
  MST_REQUIRE(list->tensors && list->chunk_map, "%s: NULL table pointer", what);
  MST_REQUIRE(list->n_tensors >= 1 && list->n_chunks >= list->n_tensors, "%s: n_tensors = %d, n_chunks = %d (every tensor has at "
              "least one chunk)", what, list->n_tensors, list->n_chunks);
  return MST_OK;
}

}  // namespace

extern "C" {

int mst_optim_chunk_elems(void) { return kChunk; }

size_t mst_optim_grad_norm_workspace_bytes(int n_chunks) { return n_chunks < 1 ? 0 : (size_t)n_chunks * sizeof(double); }

int mst_optim_grad_norm(const mst_optim_list* list, float max_norm, float* norm, float* coef, void* workspace,
                        size_t workspace_bytes, void* stream) {
  int rc = list_ok(list, "mst_optim_grad_norm");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(norm && coef && workspace, "mst_optim_grad_norm: NULL pointer");
  MST_REQUIRE(!(max_norm < 0.f), "mst_optim_grad_norm: max_norm = %g", (double)max_norm);
  if (workspace_bytes < mst_optim_grad_norm_workspace_bytes(list->n_chunks))
    return mst::fail(MST_ENOMEM, "mst_optim_grad_norm: workspace of %zu bytes, %zu needed", workspace_bytes,
                     mst_optim_grad_norm_workspace_bytes(list->n_chunks));
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(optim_sumsq_kernel, dim3(list->n_chunks), dim3(kThreads), 0, st, list->tensors, list->chunk_map, part);
  hipLaunchKernelGGL(optim_norm_fold_kernel, dim3(1), dim3(kThreads), 0, st, part, list->n_chunks, max_norm, norm, coef);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_optim_scale_grads(const mst_optim_list* list, const float* coef, void* stream) {
  int rc = list_ok(list, "mst_optim_scale_grads");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(coef, "mst_optim_scale_grads: NULL coefficient");
  hipLaunchKernelGGL(optim_scale_kernel, dim3(list->n_chunks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), list->tensors,
                     list->chunk_map, coef);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

size_t mst_optim_step_workspace_bytes(int n_tensors) { return n_tensors < 1 ? 0 : (size_t)n_tensors * sizeof(StepScalars); }

int mst_optim_step(const mst_optim_list* list, const mst_optim_hyper* hp, const float* grad_scale, const float* found_inf,
                   void* workspace, size_t workspace_bytes, void* stream) {
  int rc = list_ok(list, "mst_optim_step");
  if (rc != MST_OK) return rc;
  MST_REQUIRE(hp, "mst_optim_step: NULL hyper-parameters");
  MST_REQUIRE(hp->algo == MST_OPTIM_ADAM || hp->algo == MST_OPTIM_ADAMW || hp->algo == MST_OPTIM_SGD,
              "mst_optim_step: algo = %d (MST_OPTIM_ADAM, MST_OPTIM_ADAMW or MST_OPTIM_SGD)", hp->algo);
  MST_REQUIRE(hp->amsgrad == 0, "mst_optim_step: amsgrad is not built");
  MST_REQUIRE(hp->maximize == 0, "mst_optim_step: maximize is not built");
  MST_REQUIRE(hp->nesterov == 0, "mst_optim_step: nesterov momentum is not built");
  MST_REQUIRE(hp->dampening == 0.0, "mst_optim_step: dampening = %g is not built (0 only)", hp->dampening);
  MST_REQUIRE(hp->lr >= 0.0 && hp->lr < INFINITY, "mst_optim_step: lr = %g", hp->lr);
  MST_REQUIRE(hp->weight_decay >= 0.0 && hp->weight_decay < INFINITY, "mst_optim_step: weight_decay = %g", hp->weight_decay);
  const Hyper h{hp->lr, hp->beta1, hp->beta2, hp->eps, hp->weight_decay, hp->momentum};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(list->n_chunks), block(kThreads);
  if (hp->algo == MST_OPTIM_SGD) {
    MST_REQUIRE(hp->momentum >= 0.0 && hp->momentum < INFINITY, "mst_optim_step: momentum = %g", hp->momentum);
    hipLaunchKernelGGL(optim_step_kernel<MST_OPTIM_SGD>, grid, block, 0, st, list->tensors, list->chunk_map, h, nullptr, grad_scale,
                       found_inf);
    MST_HIP_CHECK(hipGetLastError());
    return MST_OK;
  }
  MST_REQUIRE(hp->beta1 >= 0.0 && hp->beta1 < 1.0 && hp->beta2 >= 0.0 && hp->beta2 < 1.0, "mst_optim_step: betas = (%g, %g), each in "
              "[0, 1)", hp->beta1, hp->beta2);
  MST_REQUIRE(hp->eps >= 0.0 && hp->eps < INFINITY, "mst_optim_step: eps = %g", hp->eps);
  MST_REQUIRE(workspace, "mst_optim_step: NULL workspace");
  if (workspace_bytes < mst_optim_step_workspace_bytes(list->n_tensors))
    return mst::fail(MST_ENOMEM, "mst_optim_step: workspace of %zu bytes, %zu needed", workspace_bytes,
                     mst_optim_step_workspace_bytes(list->n_tensors));
  StepScalars* sc = static_cast<StepScalars*>(workspace);
  hipLaunchKernelGGL(optim_prep_kernel, dim3((list->n_tensors + 63) / 64), dim3(64), 0, st, list->tensors, list->n_tensors, h, found_inf,
                     sc);
  if (hp->algo == MST_OPTIM_ADAM)
    hipLaunchKernelGGL(optim_step_kernel<MST_OPTIM_ADAM>, grid, block, 0, st, list->tensors, list->chunk_map, h, sc, grad_scale, found_inf);
  else
    hipLaunchKernelGGL(optim_step_kernel<MST_OPTIM_ADAMW>, grid, block, 0, st, list->tensors, list->chunk_map, h, sc, grad_scale,
                       found_inf);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_keep_best(const float* loss, float* best, int32_t* best_index, float* history, int index, const mst_keep_copy* copies,
                  int n_copies, void* stream) {
  MST_REQUIRE(loss && best && best_index, "mst_keep_best: NULL pointer");
  MST_REQUIRE(index >= 0, "mst_keep_best: index = %d", index);
  MST_REQUIRE(n_copies >= 0 && n_copies <= kMaxCopies, "mst_keep_best: %d copies (at most %d)", n_copies, kMaxCopies);
  MST_REQUIRE(n_copies == 0 || copies, "mst_keep_best: NULL copy list");
  Copies cp{};
  for (int k = 0; k < n_copies; ++k) {
    MST_REQUIRE(copies[k].src && copies[k].dst && copies[k].bytes >= 0, "mst_keep_best: copy %d: NULL pointer or negative size", k);
    MST_REQUIRE(copies[k].bytes % 4 == 0 && (uintptr_t)copies[k].src % 4 == 0 && (uintptr_t)copies[k].dst % 4 == 0,
                "mst_keep_best: copy %d: pointers and size must be multiples of 4 bytes", k);
    cp.src[k] = static_cast<const uint32_t*>(copies[k].src);
    cp.dst[k] = static_cast<uint32_t*>(copies[k].dst);
    cp.words[k] = copies[k].bytes / 4;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_copies > 0) hipLaunchKernelGGL(keep_best_copy_kernel, dim3(kCopyBlocks, n_copies), dim3(kThreads), 0, st, loss, best, cp);
  hipLaunchKernelGGL(keep_best_update_kernel, dim3(1), dim3(1), 0, st, loss, best, best_index, history, index);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
