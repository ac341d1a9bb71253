// Device helpers shared by the per-image pair kernels of sgdet.hip (test pairs), relsample.hip and gtbox_relsample.hip
// (training pairs), the box head's sampler of boxsample.hip and the RPN loss of rpnloss.hip: the reference's box IoU and box
// encoding arithmetic, the order-preserving float key, the block-wide scan of their radix selects and, for the training
// samplers, the counter-based hash, the radix select and the bitonic sort.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace veto {

// boxlist_iou(a, b)[i, j] (boxlist_ops.py:54-89) operation for operation, TO_REMOVE = 1:
// wh = clamp(min(x2) - max(x1) + 1, 0) ...; inter = w * h; inter / ((area_i + area_j) - inter)
__device__ __forceinline__ float boxlist_iou(const float* bi, const float* bj) {
#pragma clang fp contract(off)   // a last-ulp change flips `iou > thr` and `0 < iou < 1`
  const float w = fmaxf((fminf(bi[2], bj[2]) - fmaxf(bi[0], bj[0])) + 1.f, 0.f);
  const float h = fmaxf((fminf(bi[3], bj[3]) - fmaxf(bi[1], bj[1])) + 1.f, 0.f);
  const float inter = w * h;
  const float area_i = ((bi[2] - bi[0]) + 1.f) * ((bi[3] - bi[1]) + 1.f);
  const float area_j = ((bj[2] - bj[0]) + 1.f) * ((bj[3] - bj[1]) + 1.f);
  return inter / ((area_i + area_j) - inter);
}

// BoxCoder.encode of one proposal (or anchor) against one GT box (TO_REMOVE = 1), in the reference's order of operations
__device__ __forceinline__ float4 encode_box(const float4 g, const float4 p, float wx, float wy, float ww, float wh) {
#pragma clang fp contract(off)
  const float ex_w = (p.z - p.x) + 1.f, ex_h = (p.w - p.y) + 1.f;
  const float ex_cx = p.x + 0.5f * ex_w, ex_cy = p.y + 0.5f * ex_h;
  const float gt_w = (g.z - g.x) + 1.f, gt_h = (g.w - g.y) + 1.f;
  const float gt_cx = g.x + 0.5f * gt_w, gt_cy = g.y + 0.5f * gt_h;
  return make_float4((wx * (gt_cx - ex_cx)) / ex_w, (wy * (gt_cy - ex_cy)) / ex_h, ww * logf(gt_w / ex_w), wh * logf(gt_h / ex_h));
}

// order-preserving map of a float onto uint32 (larger float -> larger key, equal floats -> equal keys: -0.0 and +0.0 share the
// key of +0.0, as they compare equal in the reference's sorts and in every order documented here, which then falls through to
// the index; the raw bit pattern would put +0.0 above -0.0).  Callers: the NMS scores and RPN logits of nms.hip / rpn.hip, and
// the pair-quality products of sgdet.hip and relsample.hip, which multiply two class probabilities (>= 0) and so never see -0.0.
__device__ __forceinline__ uint32_t float_order(float f) {
  const uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// block-wide (256 threads) exclusive prefix sum; returns this thread's prefix, *total gets the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    sum += t;
  }
  __syncthreads();   // s_wave is reused by the next call
  *total = sum;
  return base + x - v;
}

// ---- counter-based random numbers and the random-subset machinery of the training samplers (relsample.hip,
// gtbox_relsample.hip): a random subset of size K is the K elements with the smallest hash, in ascending (hash, index) order
__device__ __forceinline__ uint64_t mix64(uint64_t z) {   // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t rng64(uint64_t seed, int img, int purpose, uint32_t elem) {
  const uint64_t stream = mix64(seed ^ mix64(((uint64_t)(uint32_t)img << 2) | (uint32_t)purpose));
  return mix64(stream + (uint64_t)elem * 0x9E3779B97F4A7C15ull);
}

struct SelLds {
  int hist[256];
  int wave[4];
  int digit, need;
};

// Radix select (8 bits a pass, most significant first) of the K-th largest 32-bit key among the elements `each`
// visits: each(f) calls f(key) for this thread's elements in element order, threads owning consecutive ranges in
// thread order.  Keys > T are all among the K; of the keys == T the first `need` in element order.  0 < K < count.
template <class Each>
__device__ inline void radix_select(Each each, int K, SelLds& s, uint32_t& T, int& need) {
  uint32_t prefix = 0, pmask = 0;
  need = K;
  for (int shift = 24; shift >= 0; shift -= 8) {
    s.hist[threadIdx.x] = 0;
    __syncthreads();
    each([&](uint32_t k) {
      if ((k & pmask) == prefix) atomicAdd(&s.hist[(k >> shift) & 255], 1);
    });
    __syncthreads();
    const int h = s.hist[255 - threadIdx.x];   // an ascending scan over descending digits
    int dummy;
    const int above = block_exclusive_scan(h, s.wave, &dummy);
    if (above < need && above + h >= need) { s.digit = 255 - threadIdx.x; s.need = need - above; }
    __syncthreads();
    prefix |= (uint32_t)s.digit << shift;
    pmask |= 255u << shift;
    need = s.need;
    __syncthreads();
  }
  T = prefix;
}

// this thread's rank among the keys == T (element order): the exclusive scan of its own count
template <class Each>
__device__ inline int equal_rank(Each each, uint32_t T, SelLds& s) {
  int eq = 0;
  each([&](uint32_t k) { eq += k == T; });
  int dummy;
  return block_exclusive_scan(eq, s.wave, &dummy);
}

// ascending bitonic sort of key[0..cnt) by the whole block; the array is padded to the next power of two with ~0, so it
// must hold that many elements
__device__ inline void bitonic_sort(unsigned long long* key, int cnt) {
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  for (int t = cnt + threadIdx.x; t < n2; t += blockDim.x) key[t] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n2; t += blockDim.x) {
        const int l = t ^ j;
        if (l > t) {
          const unsigned long long kt = key[t], kl = key[l];
          const bool up = (t & k) == 0;
          if (up ? kt > kl : kt < kl) { key[t] = kl; key[l] = kt; }
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace veto
