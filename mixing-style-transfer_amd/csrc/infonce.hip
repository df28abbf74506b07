// InfoNCE forward on (all-gathered) embeddings.  Replaces InfoNCELoss.forward src/loss.py:31-136:
//   E = normalize(E); S = E E^T / tau; row-max subtraction; pos_i = sum_{j != i, lab_j == lab_i} exp(S_ij),
//   neg_i = sum_{lab_j != lab_i} exp(S_ij); loss_i = -log(pos_i / (pos_i + neg_i + 1e-8)) for anchors with pos_i > 0.
// One workgroup per local anchor row; no host sync per anchor (the reference syncs N times).
// Backward: d(scale * sum_i loss_i)/dE for all N rows, what autograd derives from the lines above:
//   c_ij = dloss_i/dS_ij = e_ij [j != i] / (pos_i + neg_i + 1e-8) - e_ij [j != i, lab_j == lab_i] / pos_i,
//   dL/de_n = (sum_j c_nj e_j [n local] + sum_i c_in e_i) / tau,  dL/dE_n = (g - e_n (e_n . g)) / |E_n|.
// (The row-max subtraction contributes 1e-8 / (pos + neg + 1e-8) to the arg-max column: below fp32 resolution of
// c_ij, dropped.)
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void l2norm_kernel(const float* emb, float* inv_norm, int D) {
  __shared__ float red[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  float a = 0.f;
  for (int d = tid; d < D; d += 256) {
    const float v = emb[(size_t)r * D + d];
    a = fmaf(v, v, a);
  }
  a = mst::wave_sum(a);
  if ((tid & 63) == 0) red[tid >> 6] = a;
  __syncthreads();
  if (tid == 0) inv_norm[r] = 1.0f / fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-12f);  // F.normalize eps
}

// Forward: two launches (three before).  Workgroup = one local anchor row i: every wave forms the inverse norms it needs itself
// (its own columns' and the anchor's, from the same loads as the dot products; a wave's sum of squares is 64 strided partial
// sums met in wave_sum's tree, the same bits in whichever workgroup or wave computes it), writes S_i. and the row's
// (loss, has-positive) pair; infonce_reduce_kernel adds the pairs in a fixed tree.  No float atomics, no state between
// workgroups or between calls: the loss is bit-identical from run to run (the reference's deterministic mode, src/train.py:30).
// (Folding the reduction into this launch needs an arrival counter that is zero at every start: a memset node per call, i.e. the
// launch it would save, or state outside the caller's workspace, which the ABI rules out.  Tried with library-owned counters,
// 23.3 us for the single launch; dropped for that reason.)
constexpr int kInfoThreads = 512, kInfoWaves = kInfoThreads / 64;
__global__ __launch_bounds__(kInfoThreads) void infonce_fwd_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                                   float* sim, int N, int D, int row0, float inv_tau, float* rowout) {
  extern __shared__ float srow[];  // [D] normalised anchor
  __shared__ float red[3 * kInfoWaves];
  const int i = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto inv_of = [](float sumsq) { return 1.0f / fmaxf(sqrtf(sumsq), 1e-12f); };   // F.normalize eps
  {
    float q = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float v = emb[(size_t)i * D + d];
      q = fmaf(v, v, q);
    }
    const float ni = inv_of(mst::wave_sum(q));   // (every wave: the same bits)
    for (int d = tid; d < D; d += kInfoThreads) srow[d] = emb[(size_t)i * D + d] * ni;
  }
  __syncthreads();
  float* s = sim + (size_t)blockIdx.x * N;
  float mx = -INFINITY;
  for (int j0 = wave * 4; j0 < N; j0 += 4 * kInfoWaves) {  // one wave = 4 columns at a time: 4 independent coalesced dot products
    float a[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
    const float* ej[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ej[u] = emb + (size_t)min(j0 + u, N - 1) * D;
#pragma unroll 4
    for (int d = lane; d < D; d += 64) {
      const float x = srow[d];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float v = ej[u][d];
        a[u] = fmaf(x, v, a[u]);
        q[u] = fmaf(v, v, q[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j >= N) break;
      const float v = mst::wave_sum(a[u]) * inv_of(mst::wave_sum(q[u])) * inv_tau;
      if (lane == 0) s[j] = v;
      mx = fmaxf(mx, v);
    }
  }
  if (lane == 0) red[wave] = mx;
  __syncthreads();   // (also orders the lane-0 stores of s[] before the reads below: same workgroup, same L1)
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kInfoWaves; ++w) mx = fmaxf(mx, red[w]);
  const int64_t li = labels[i];
  float pos = 0.f, neg = 0.f;
  for (int j = tid; j < N; j += kInfoThreads) {
    const float e = expf(s[j] - mx);
    const bool same = labels[j] == li;
    if (same && j != i) pos += e;
    if (!same) neg += e;
  }
  pos = mst::wave_sum(pos), neg = mst::wave_sum(neg);
  if (lane == 0) red[kInfoWaves + wave] = pos, red[2 * kInfoWaves + wave] = neg;
  __syncthreads();
  if (tid == 0) {
    pos = neg = 0.f;
#pragma unroll
    for (int w = 0; w < kInfoWaves; ++w) pos += red[kInfoWaves + w], neg += red[2 * kInfoWaves + w];
    rowout[2 * blockIdx.x] = pos > 0.f ? -logf(pos / (pos + neg + 1e-8f)) : 0.f;
    rowout[2 * blockIdx.x + 1] = pos > 0.f ? 1.0f : 0.f;
  }
}

// out[0] = sum of the per-anchor losses, out[1] = number of anchors with a positive: fixed-shape tree, fixed order
__global__ __launch_bounds__(256) void infonce_reduce_kernel(const float* rowout, int rows, float* out) {
  __shared__ float sl[256], sc[256];
  const int tid = threadIdx.x;
  float l = 0.f, c = 0.f;
  for (int r = tid; r < rows; r += 256) l += rowout[2 * r], c += rowout[2 * r + 1];
  sl[tid] = l, sc[tid] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sl[tid] += sl[tid + o], sc[tid] += sc[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = sl[0], out[1] = sc[0];
}

// rows kernel of the backward pass: recomputes S_i., then overwrites it with the coefficients c_i.
// The scores, their exponentials and the two sums are formed in double from the raw rows (norms included): the coefficients are
// softmax weights of scores up to 1 / tau, so an fp32 score carries 2^-24 / tau into every c_ij, and the gradient is a sum of
// c_ij e_j that the normalisation then projects most of away (at D = 3 the fp32 coefficients put the gradient at twice the fp32
// oracle's own distance from float64).  c_ij itself is stored in fp32.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ __launch_bounds__(256) void infonce_coef_kernel(const float* emb, const int64_t* labels, float* coef, int N, int D,
                                                           int row0, float inv_tau) {
  extern __shared__ float srow[];   // [D] the anchor row (raw)
  __shared__ double red[12];
  double* sc = reinterpret_cast<double*>(srow + ((D + 1) & ~1));   // [N] scores -> exponentials
  const int i = row0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int d = tid; d < D; d += 256) srow[d] = emb[(size_t)i * D + d];
  __syncthreads();
  auto inv_of = [](double sumsq) { return 1.0 / fmax(sqrt(sumsq), 1e-12); };   // F.normalize eps
  double qi = 0.0;
  for (int d = lane; d < D; d += 64) qi = fma((double)srow[d], (double)srow[d], qi);
  const double ni = inv_of(wave_sum_d(qi));   // (every wave: the same bits)
  float* s = coef + (size_t)blockIdx.x * N;
  double mx = -INFINITY;
  for (int j0 = wave * 4; j0 < N; j0 += 16) {
    double a[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    const float* ej[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ej[u] = emb + (size_t)min(j0 + u, N - 1) * D;
    for (int d = lane; d < D; d += 64) {
      const double x = (double)srow[d];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double v = (double)ej[u][d];
        a[u] = fma(x, v, a[u]);
        q[u] = fma(v, v, q[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u;
      if (j >= N) break;
      const double v = wave_sum_d(a[u]) * ni * inv_of(wave_sum_d(q[u])) * (double)inv_tau;
      if (lane == 0) sc[j] = v;
      mx = fmax(mx, v);
    }
  }
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  const int64_t li = labels[i];
  double pos = 0.0, neg = 0.0;
  for (int j = tid; j < N; j += 256) {
    const double e = exp(sc[j] - mx);
    sc[j] = e;   // (only this thread touches column j from here on)
    const bool same = labels[j] == li;
    if (same && j != i) pos += e;
    if (!same) neg += e;
  }
  pos = wave_sum_d(pos), neg = wave_sum_d(neg);
  if (lane == 0) red[4 + wave] = pos, red[8 + wave] = neg;
  __syncthreads();
  pos = (red[4] + red[5]) + (red[6] + red[7]);
  neg = (red[8] + red[9]) + (red[10] + red[11]);
  const bool has_pos = (float)pos > 0.f;   // the forward's test, on its fp32 sum
  const double inv_den = 1.0 / (pos + neg + 1e-8), inv_pos = has_pos ? 1.0 / pos : 0.0;
  for (int j = tid; j < N; j += 256) {
    const double e = sc[j];
    const bool same = labels[j] == li;
    double c = 0.0;
    if (has_pos && j != i) c = e * inv_den - (same ? e * inv_pos : 0.0);
    s[j] = (float)c;
  }
}

// one workgroup per embedding row n: g = (sum_j c_nj e_j [n local] + sum_i c_in e_i) / tau, then through F.normalize
__global__ __launch_bounds__(256) void infonce_grad_kernel(const float* emb, const float* inv_norm, const float* coef,
                                                           const float* scale, float* grad, int N, int D, int row0,
                                                           int rows, float inv_tau) {
  extern __shared__ float sg[];   // [D] gradient w.r.t. the normalised row
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const bool local = n >= row0 && n < row0 + rows;
  const float* crow = coef + (local ? (size_t)(n - row0) * N : 0);
  float dot = 0.f;
  const float nn = inv_norm[n];
  for (int d = tid; d < D; d += 256) {
    // up to 2 N signed terms that largely cancel: accumulated in double and rounded once (an fp32 chain of that length is
    // 2.4 x as far from float64 as a blocked fp32 matrix product at N = 384, D = 768)
    double acc = 0.0;
    if (local)
      for (int j = 0; j < N; ++j) acc = fma((double)crow[j], (double)(emb[(size_t)j * D + d] * inv_norm[j]), acc);
    for (int i = 0; i < rows; ++i)
      acc = fma((double)coef[(size_t)i * N + n], (double)(emb[(size_t)(row0 + i) * D + d] * inv_norm[row0 + i]), acc);
    const float g = (float)acc * inv_tau;
    sg[d] = g;
    dot = fmaf(g, emb[(size_t)n * D + d] * nn, dot);
  }
  dot = mst::wave_sum(dot);
  if ((tid & 63) == 0) red[tid >> 6] = dot;
  __syncthreads();
  dot = (red[0] + red[1]) + (red[2] + red[3]);
  const float sc = scale ? *scale : 1.0f;
  for (int d = tid; d < D; d += 256) grad[(size_t)n * D + d] = sc * (nn * (sg[d] - emb[(size_t)n * D + d] * nn * dot));   // the incoming factor last: k x the gradient to one rounding
}

}  // namespace

extern "C" {

size_t mst_infonce_workspace_bytes(int N, int D) {
  if (N <= 0 || D <= 0) return 0;
  return mst::align_up((size_t)N * sizeof(float), 256) + mst::align_up((size_t)N * N * sizeof(float), 256) +
         mst::align_up((size_t)2 * N * sizeof(float), 256);
}

int mst_infonce_forward(const float* emb, const int64_t* labels, int N, int D, int row0, int rows, float temperature,
                        float* out, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(emb && labels && out, "mst_infonce_forward: NULL argument");
  MST_REQUIRE(N > 0 && D > 0 && row0 >= 0 && rows > 0 && row0 + rows <= N && temperature > 0.f,
              "mst_infonce_forward: bad sizes N=%d D=%d row0=%d rows=%d", N, D, row0, rows);
  const size_t need = mst_infonce_workspace_bytes(N, D);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_infonce_forward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // (the workspace's first region, N floats, holds the inverse norms of the backward pass; the forward forms its own in registers)
  float* sim = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + mst::align_up((size_t)N * sizeof(float), 256));
  float* rowout = reinterpret_cast<float*>(reinterpret_cast<char*>(sim) + mst::align_up((size_t)N * N * sizeof(float), 256));
  hipLaunchKernelGGL(infonce_fwd_kernel, dim3(rows), dim3(kInfoThreads), (size_t)D * sizeof(float), st, emb, labels, sim, N, D, row0,
                     1.0f / temperature, rowout);
  hipLaunchKernelGGL(infonce_reduce_kernel, dim3(1), dim3(256), 0, st, rowout, rows, out);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

int mst_infonce_backward(const float* emb, const int64_t* labels, int N, int D, int row0, int rows, float temperature,
                         const float* scale, float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  MST_REQUIRE(emb && labels && grad, "mst_infonce_backward: NULL argument");
  MST_REQUIRE(N > 0 && D > 0 && row0 >= 0 && rows > 0 && row0 + rows <= N && temperature > 0.f,
              "mst_infonce_backward: bad sizes N=%d D=%d row0=%d rows=%d", N, D, row0, rows);
  // infonce_coef_kernel keeps the anchor row and N scores (double) in dynamic LDS
  const size_t coef_lds = (size_t)((D + 1) & ~1) * sizeof(float) + (size_t)N * sizeof(double);
  MST_REQUIRE(coef_lds <= 64 * 1024, "mst_infonce_backward: 4 D + 8 N = %zu B of LDS, limit 65536 (N=%d D=%d)", coef_lds, N, D);
  const size_t need = mst_infonce_workspace_bytes(N, D);
  if (!workspace || workspace_bytes < need)
    return mst::fail(MST_ENOMEM, "mst_infonce_backward: workspace %zu B < required %zu B", workspace_bytes, need);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* inv_norm = reinterpret_cast<float*>(workspace);
  float* coef = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + mst::align_up((size_t)N * sizeof(float), 256));
  hipLaunchKernelGGL(l2norm_kernel, dim3(N), dim3(256), 0, st, emb, inv_norm, D);
  hipLaunchKernelGGL(infonce_coef_kernel, dim3(rows), dim3(256), coef_lds, st, emb, labels, coef, N, D, row0, 1.0f / temperature);
  hipLaunchKernelGGL(infonce_grad_kernel, dim3(N), dim3(256), (size_t)D * sizeof(float), st, emb, inv_norm, coef, scale,
                     grad, N, D, row0, rows, 1.0f / temperature);
  MST_HIP_CHECK(hipGetLastError());
  return MST_OK;
}

}  // extern "C"
