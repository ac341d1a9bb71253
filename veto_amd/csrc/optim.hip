// The optimizer side of a training iteration: clip_grad_norm (pysgg/utils/checkpoint.py:180-219) and the step of the
// torch.optim.Adam that make_optimizer returns (pysgg/solver/build.py:7-34), over every parameter tensor at once.  The reference
// launches one norm per parameter, reads the coefficient back to decide whether to clip, launches one mul_ per parameter and
// then steps one param group, that is one tensor, at a time.  Here a table of tensors and a table of chunks (kOptimChunk elements
// of one tensor per workgroup) drive two kernels, whatever the number of tensors:
//
//   optim_norm_kernel       one workgroup per chunk: the sum of g^2, every g converted to double before it is squared, a fixed
//                           element-to-thread assignment, then shuffles and four wave sums in wave order.  The sum goes to the
//                           workspace; the workgroup then counts itself out on an integer counter, and the workgroup that counts
//                           last folds the partials: per tensor in chunk order, then the tensors in the order of
//                           box_loss_final_kernel (thread t the tensors [t ceil(n / 256), (t + 1) ceil(n / 256)), then the 256
//                           sums in thread order).  Which workgroup folds varies, what it computes does not: two calls give the
//                           same bits.  No floating-point atomic.  It writes the norms, the total and the applied coefficient.
//   optim_apply_kernel<M>   one workgroup per chunk.  M = 1: g *= coef in place (nothing is touched when coef is exactly 1).
//                           M = 2: the Adam step, with the gradient scaled in registers by the coefficient read from device memory
//                           (or by exactly 1) and left as it is in memory.
//
// 16-byte accesses where every pointer the kernel uses for the tensor is 16-byte aligned (a chunk starts at a multiple of
// kOptimChunk elements, so it keeps the tensor's alignment), 4-byte accesses for the whole chunk otherwise and for the tail.
#include "common.h"
#include "kernels.h"

namespace veto {

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(256) void optim_norm_kernel(OptimArgs a) {
  __shared__ double s_wave[4];
  __shared__ double s_sum[256];
  __shared__ int s_last;
  const int tid = threadIdx.x, c = blockIdx.x;
  if (c < a.n_chunks) {
    const OptimChunk ch = a.chunks[c];
    const OptimTensor& t = a.tensors[ch.tensor];
    const long long start = (long long)ch.index * kOptimChunk;
    const int len = (int)min((long long)kOptimChunk, (long long)t.numel - start);
    const float* g = t.g + start;
    double acc = 0.0;
    int done = 0;
    if (aligned16(g)) {
      const int n4 = len >> 2;
      const float4* g4 = reinterpret_cast<const float4*>(g);
      for (int i = tid; i < n4; i += 256) {
        const float4 x = g4[i];
        acc += sq(x.x);
        acc += sq(x.y);
        acc += sq(x.z);
        acc += sq(x.w);
      }
      done = n4 << 2;
    }
    for (int i = done + tid; i < len; i += 256) acc += sq(g[i]);
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) s_wave[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      const double sum = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
      __hip_atomic_store(&a.partial[c], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid == 0) {
    __threadfence();   // the partial before the count
    s_last = atomicAdd(a.counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();     // the count before every other workgroup's partial

  for (int i = tid; i < a.n_tensors; i += 256) {
    const OptimTensor& t = a.tensors[i];
    double s = 0.0;
    for (int k = 0; k < t.n_chunks; ++k) s += __hip_atomic_load(&a.partial[t.chunk0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.tensor_sq[i] = s;
    a.norms[i] = (float)sqrt(s);
  }
  __syncthreads();
  const int per = (a.n_tensors + 255) / 256;
  double s = 0.0;
  for (int i = tid * per; i < (tid + 1) * per && i < a.n_tensors; ++i) s += a.tensor_sq[i];
  s_sum[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int t = 0; t < 256; ++t) tot += s_sum[t];
    const double total = sqrt(tot);
    const float coef = (float)(a.max_norm / (total + 1e-6));   // checkpoint.py:207, in double, rounded once
    a.total[0] = (float)total;
    a.coef[0] = coef < 1.f ? coef : 1.f;                       // checkpoint.py:208; NaN < 1 is false
  }
}

struct AdamLane {
  float coef, wd, beta1, omb1, beta2, omb2, eps, step_size, bc2_sqrt;
  // torch/optim/adam.py, _single_tensor_adam without amsgrad, maximize, capturable or differentiable
  __device__ __forceinline__ void operator()(float& p, float g, float& m, float& v) const {
    // g', m and v are formed in double from the fp32 operands and rounded to fp32 once each: the pass is a memory stream (the
    // fp64 work did not show in the kernel's measured time), and m and v then carry one rounding instead of four (against the float64 step: 4u where fp32 fmas
    // reach 9u).  Explicit fmas: the roundings do not depend on the compiler's contraction setting.
    double gd = (double)coef * (double)g;
    if (wd != 0.f) gd = fma((double)wd, (double)p, gd);                 // grad.add(param, alpha=weight_decay), skipped at 0 as torch skips it
    m = (float)fma((double)omb1, gd, (double)beta1 * (double)m);         // exp_avg.lerp_(grad, 1 - beta1)
    v = (float)fma((double)omb2 * gd, gd, (double)beta2 * (double)v);    // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = fmaf(-step_size, m / denom, p);          // param.addcdiv_(exp_avg, denom, value=-step_size)
  }
};

template <int MODE>   // 1: scale the gradients in place; 2: the Adam step
__global__ __launch_bounds__(256) void optim_apply_kernel(OptimArgs a, int use_coef) {
  const float coef = use_coef ? a.coef[0] : 1.f;
  if (MODE == 1 && coef == 1.f) return;          // checkpoint.py:208: no mul_ unless clip_coef < 1
  const int tid = threadIdx.x;
  const OptimChunk ch = a.chunks[blockIdx.x];
  const OptimTensor& t = a.tensors[ch.tensor];
  const long long start = (long long)ch.index * kOptimChunk;
  const int len = (int)min((long long)kOptimChunk, (long long)t.numel - start);
  float* g = const_cast<float*>(t.g) + start;
  if (MODE == 1) {
    int done = 0;
    if (aligned16(g)) {
      const int n4 = len >> 2;
      float4* g4 = reinterpret_cast<float4*>(g);
      for (int i = tid; i < n4; i += 256) {
        float4 x = g4[i];
        x.x *= coef; x.y *= coef; x.z *= coef; x.w *= coef;
        g4[i] = x;
      }
      done = n4 << 2;
    }
    for (int i = done + tid; i < len; i += 256) g[i] *= coef;
    return;
  }
  float *p = t.p + start, *m = t.m + start, *v = t.v + start;
  const AdamLane f{coef, t.wd, t.beta1, t.omb1, t.beta2, t.omb2, t.eps, t.step_size, t.bc2_sqrt};
  int done = 0;
  if (aligned16(g) && aligned16(p) && aligned16(m) && aligned16(v)) {
    const int n4 = len >> 2;
    float4 *p4 = reinterpret_cast<float4*>(p), *m4 = reinterpret_cast<float4*>(m), *v4 = reinterpret_cast<float4*>(v);
    const float4* g4 = reinterpret_cast<const float4*>(g);
#pragma unroll 2
    for (int i = tid; i < n4; i += 256) {
      float4 pp = p4[i], mm = m4[i], vv = v4[i];
      const float4 gg = g4[i];
      f(pp.x, gg.x, mm.x, vv.x);
      f(pp.y, gg.y, mm.y, vv.y);
      f(pp.z, gg.z, mm.z, vv.z);
      f(pp.w, gg.w, mm.w, vv.w);
      p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    done = n4 << 2;
  }
  for (int i = done + tid; i < len; i += 256) {
    float pp = p[i], mm = m[i], vv = v[i];
    f(pp, g[i], mm, vv);
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}

}  // namespace

hipError_t launch_optim(const OptimArgs& a, bool norms, int apply, bool use_coef, hipStream_t s) {
  if (a.n_tensors < 1 || a.n_tensors > kOptimMaxTensors || a.n_chunks < 0 || a.n_chunks > kOptimMaxChunks || apply < 0 || apply > 2)
    return hipErrorInvalidValue;
  if (norms) {   // no chunk at all: one workgroup that only folds (every norm 0)
    VETO_LAUNCH(optim_norm_kernel, dim3(a.n_chunks > 0 ? a.n_chunks : 1), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (apply == 0 || a.n_chunks == 0) return hipSuccess;
  if (apply == 1) VETO_LAUNCH(optim_apply_kernel<1>, dim3(a.n_chunks), dim3(256), 0, s, a, use_coef ? 1 : 0);
  else VETO_LAUNCH(optim_apply_kernel<2>, dim3(a.n_chunks), dim3(256), 0, s, a, use_coef ? 1 : 0);
  return hipGetLastError();
}

}  // namespace veto
