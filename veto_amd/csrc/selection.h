// Device helpers shared by the per-image pair kernels of sgdet.hip (test pairs) and relsample.hip (training pairs):
// the reference's box IoU arithmetic, the order-preserving float key and the block-wide scan of their radix selects.
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

// order-preserving map of a float onto uint32 (larger float -> larger key)
__device__ __forceinline__ uint32_t float_order(float f) {
  const uint32_t u = __float_as_uint(f);
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

}  // namespace veto
