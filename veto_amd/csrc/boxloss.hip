// Detector training, the box head's loss: FastRCNNLossComputation.__call__ (pysgg/modeling/roi_heads/box_head/loss.py:42-84) over
// the R rows FastRCNNSampling.subsample kept.  The reference concatenates per-image lists, runs a nonzero over labels > 0 whose
// count is read back, gathers [P, 4] out of [R, 4C] by advanced indexing and, in its backward, scatters into a zero-filled
// [R, 4C]: some twenty launches and one device->host synchronisation for two scalars.  Here R = labels.numel() is known on the
// host, so nothing has to be counted before a gradient can be written, and one pass does it.  Two launches whatever R and C:
//
//   box_loss_rows_kernel<K>  one wave per row, four rows per workgroup (the shape of ce_rows_kernel).  The row's C <= 64 K logits
//                            are read once, in place through their row stride, and stay in registers; the maximum and the sum go
//                            through wave shuffles and the maximum is subtracted before any exponential.  The terms are formed in
//                            double from the fp32 inputs: lse - z[y], and for y > 0 the four smooth-L1 terms (beta 1) of columns
//                            4y..4y+3 (4..7 when class-agnostic) against the row's targets.  Two doubles per row go to the
//                            workspace.  When gradients are asked for the same wave writes (softmax - onehot) / R and the WHOLE
//                            box row: zeros with 16-byte stores except clamp(d, -1, 1) / R at the four columns.  A label outside
//                            [0, C) reads nothing out of bounds: the row's partials and both its gradient rows are NaN.
//   box_loss_final_kernel    one workgroup folds the partials in row order, in double (the shape of ce_reduce_kernel), and writes
//                            the two means.  R = 0: NaN, the mean of nothing.
// No atomics, no LDS in the row kernel, no scratch; two calls give the same bits.
#include "common.h"
#include "kernels.h"

namespace veto {

namespace {

constexpr int kMaxCls = 1024;          // 16 logits per lane
constexpr int kMaxRows = 1 << 20;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int K>
__global__ __launch_bounds__(256) void box_loss_rows_kernel(BoxLossArgs a) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= a.n_rows) return;
  const int C = a.n_cls;
  const float* z = a.logits + (size_t)r * a.ld_logits;
  float v[K];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < C ? z[c] : -INFINITY;
    mx = fmaxf(mx, v[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));

  const long long yl = a.labels[r];
  const bool valid = yl >= 0 && yl < C;
  const int y = valid ? (int)yl : 0;

  double e[K], sum = 0.0;
  float zy_lane = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    e[k] = exp((double)v[k] - (double)mx);   // a padding lane or a -inf logit: exactly 0
    sum += e[k];
    if (lane + 64 * k == y) zy_lane = v[k];
  }
  sum = wave_sum_f64(sum);
  const float zy = __shfl(zy_lane, y & 63, 64);
  const double nan = __builtin_nan("");
  const double ce = valid ? ((double)mx + log(sum)) - (double)zy : nan;

  // the box term: every lane forms the same four values (the addresses are wave-uniform)
  const bool pos = valid && y > 0;
  const int col = a.cls_agnostic ? 4 : 4 * y;
  double box = valid ? 0.0 : nan;
  float gb[4] = {0.f, 0.f, 0.f, 0.f};
  const double inv = 1.0 / (double)a.n_rows;
  if (pos) {
    const float4 t4 = reinterpret_cast<const float4*>(a.targets)[r];
    const float t[4] = {t4.x, t4.y, t4.z, t4.w};
    const float* x = a.reg + (size_t)r * a.ld_reg + col;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double d = (double)x[c] - (double)t[c], ad = fabs(d);
      box += ad < 1.0 ? 0.5 * d * d : ad - 0.5;
      gb[c] = (float)(fmin(fmax(d, -1.0), 1.0) * inv);   // d below beta, sign(d) from it on: they agree at |d| = 1
    }
  }
  if (lane == 0) {
    a.partial[2 * (size_t)r] = ce;
    a.partial[2 * (size_t)r + 1] = box;
  }
  if (!a.d_logits) return;

  float* gz = a.d_logits + (size_t)r * C;
  const double scale = valid ? inv / sum : nan;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int c = lane + 64 * k;
    if (c < C) gz[c] = valid ? (float)(e[k] * scale - (c == y ? inv : 0.0)) : __builtin_nanf("");
  }
  float4* gr = reinterpret_cast<float4*>(a.d_reg + (size_t)r * a.n_reg_cols);
  const float fill = valid ? 0.f : __builtin_nanf("");
  const int hot = pos ? col >> 2 : -1;
  for (int j = lane; j < (a.n_reg_cols >> 2); j += 64)
    gr[j] = j == hot ? make_float4(gb[0], gb[1], gb[2], gb[3]) : make_float4(fill, fill, fill, fill);
}

__global__ __launch_bounds__(256) void box_loss_final_kernel(BoxLossArgs a) {
  __shared__ double s_ce[256], s_box[256];
  const int tid = threadIdx.x;
  const int per = (a.n_rows + 255) / 256;
  double ce = 0.0, box = 0.0;
  for (long long i = (long long)tid * per; i < (long long)(tid + 1) * per && i < a.n_rows; ++i) {
    ce += a.partial[2 * i];
    box += a.partial[2 * i + 1];
  }
  s_ce[tid] = ce;
  s_box[tid] = box;
  __syncthreads();
  if (tid == 0) {
    double c2 = 0.0, b2 = 0.0;
    for (int t = 0; t < 256; ++t) { c2 += s_ce[t]; b2 += s_box[t]; }
    const bool none = a.n_rows == 0;   // the mean of nothing: the reference gives NaN and 0/0
    a.losses[0] = none ? __builtin_nanf("") : (float)(c2 / (double)a.n_rows);
    a.losses[1] = none ? __builtin_nanf("") : (float)(b2 / (double)a.n_rows);
  }
}

}  // namespace

int box_loss_max_cls() { return kMaxCls; }
int box_loss_max_rows() { return kMaxRows; }

hipError_t launch_box_loss(const BoxLossArgs& a, hipStream_t s) {
  if (a.n_rows < 0 || a.n_rows > kMaxRows || a.n_cls < 2 || a.n_cls > kMaxCls) return hipErrorInvalidValue;
  const dim3 grid(a.n_rows > 0 ? (a.n_rows + 3) / 4 : 1), block(256);   // R = 0: one workgroup whose waves all leave
  if (a.n_cls <= 64) VETO_LAUNCH(box_loss_rows_kernel<1>, grid, block, 0, s, a);
  else if (a.n_cls <= 128) VETO_LAUNCH(box_loss_rows_kernel<2>, grid, block, 0, s, a);
  else if (a.n_cls <= 256) VETO_LAUNCH(box_loss_rows_kernel<4>, grid, block, 0, s, a);
  else VETO_LAUNCH(box_loss_rows_kernel<16>, grid, block, 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  VETO_LAUNCH(box_loss_final_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
