// ROI feature extraction in front of the predictor: the legacy ("aligned =
// False") ROIAlign of pysgg/csrc/cuda/ROIAlign_cuda.cu:16-125 with the FPN level choice of
// LevelMapper (pysgg/modeling/poolers.py:17-43) and Pooler.forward's cat_all_levels=False dispatch
// (poolers.py:109-171) folded into ONE launch: blockIdx.z = 0 pools every ROI from its own FPN level,
// blockIdx.z = 1 pools the depth map with the fixed 1/16 pooler.
//
// Mapping: one workgroup per (ROI, 32-channel slab).  The bilinear weights are separable, so the ROI's
// sample table is 2 x (pooled * grid) axis entries (low/high index, low/high weight, validity) built once
// in LDS and shared by every channel -- the reference recomputes it per output element.  A wave then
// owns one channel plane at a time: its 64 lanes are the 64 output bins, so the 16 taps of a lane fall
// in the ROI's footprint of ONE plane (L1/L2 resident after the first touch) and the store is one
// contiguous 256-byte row of the [R, C, 8, 8] output.  pooled 9..16 (WALK): a lane walks the bins lane, lane + 64, ...
// (ceil(P*P / 64) <= 4 of them), every pass of a wave stores the next contiguous 256 bytes of the [R, C, P, P] output; the
// instantiation for pooled <= 8 is the one-bin-per-lane code.
//
// Arithmetic: float32 in the reference's operation order with FMA contraction switched off, so the result
// is bit-identical to the CPU restatement in oracle/roi_align_oracle.py.
#include "common.h"
#include "kernels.h"

// The compiler contracts a*b + c into an FMA by default; the oracle (numpy) rounds every product.  Switch
// contraction off for the code of this file and use plain operators: hip's rounded-op intrinsics are inline
// header functions compiled under the DEFAULT contraction mode, so their results still get fused.
#pragma clang fp contract(off)

namespace veto {

namespace {

constexpr int kMaxAxis = 32;   // pooled * sampling_ratio <= 32
constexpr int kSlab = 32;      // channels per workgroup

struct AxisTable {
  int lo[kMaxAxis], hi[kMaxAxis];
  float l[kMaxAxis], h[kMaxAxis];
  int valid[kMaxAxis];
};

// one axis entry, ROIAlign_cuda.cu:21-57 restricted to one coordinate
__device__ __forceinline__ void axis_entry(AxisTable& t, int k, float start, float bin, int p, int i, int grid, int size) {
  float v = (start + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)grid;
  const bool valid = !(v < -1.0f || v > (float)size);
  if (v <= 0.f) v = 0.f;
  int lo = (int)v, hi;
  if (lo >= size - 1) {
    hi = lo = size - 1;
    v = (float)lo;
  } else {
    hi = lo + 1;
  }
  const float l = v - (float)lo;
  t.lo[k] = valid ? lo : 0;
  t.hi[k] = valid ? hi : 0;
  t.l[k] = l;
  t.h[k] = 1.0f - l;
  t.valid[k] = valid;
}

template <int G, bool WALK>  // G = sampling ratio (samples per bin and axis); WALK: pooled > 8, a lane owns several bins
__global__ __launch_bounds__(256) void roi_pool_kernel(RoiPoolArgs a) {
  __shared__ AxisTable ty, tx;
  __shared__ int s_level;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;

  if (tid == 0) {
    int lvl = 0;
    if (a.n_levels > 1) {
      // LevelMapper: floor(4 + log2(sqrt(area) / 224 + 1e-6)) clamped to [k_min, k_max], minus k_min; the
      // area uses the +1 pixel convention of BoxList.area() (bounding_box.py:249-259)
      const float area = ((roi[3] - roi[1]) + 1.f) * ((roi[4] - roi[2]) + 1.f);
      const float s = sqrtf(area);
      float t = floorf(4.f + log2f(s / 224.f + 1e-6f));
      t = fminf(fmaxf(t, (float)a.k_min), (float)a.k_max);
      lvl = (int)t - a.k_min;
    }
    s_level = lvl;
    if (a.out_levels && !depth && blockIdx.y == 0) a.out_levels[r] = lvl;
  }
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  const int P = a.pooled, n_axis = P * G;
  if (tid < 2 * n_axis) {
    const bool is_y = tid < n_axis;
    const int k = is_y ? tid : tid - n_axis;
    // :84-98 no rounding of the scaled box; malformed ROIs become 1x1
    const float lo_c = (is_y ? roi[2] : roi[1]) * L.scale;
    const float hi_c = (is_y ? roi[4] : roi[3]) * L.scale;
    const float len = fmaxf(hi_c - lo_c, 1.0f);
    const float bin = len / (float)P;
    axis_entry(is_y ? ty : tx, k, lo_c, bin, k / G, k % G, G, is_y ? L.H : L.W);
  }
  __syncthreads();

  const int b = (int)roi[0];
  const int wv = tid >> 6;
  const int n_pass = WALK ? (P * P + 63) / 64 : 1;
  for (int pass = 0; pass < n_pass; ++pass) {
    const int bin_id = pass * 64 + (tid & 63);
    const int ph = bin_id / P, pw = bin_id % P;
    if (bin_id >= P * P) return;
    // this lane's G x G samples: 4 tap offsets and 4 weights each, fixed for every channel
    int off[G * G][4];
    float wgt[G * G][4];
    bool ok[G * G];
#pragma unroll
    for (int iy = 0; iy < G; ++iy)
#pragma unroll
      for (int ix = 0; ix < G; ++ix) {
        const int ky = ph * G + iy, kx = pw * G + ix, q = iy * G + ix;
        ok[q] = ty.valid[ky] && tx.valid[kx];  // otherwise bilinear_interpolate returns 0 (:26-29)
        const float hy = ty.h[ky], ly = ty.l[ky], hx = tx.h[kx], lx = tx.l[kx];
        off[q][0] = ty.lo[ky] * L.W + tx.lo[kx];
        off[q][1] = ty.lo[ky] * L.W + tx.hi[kx];
        off[q][2] = ty.hi[ky] * L.W + tx.lo[kx];
        off[q][3] = ty.hi[ky] * L.W + tx.hi[kx];
        wgt[q][0] = hy * hx;  // :61
        wgt[q][1] = hy * lx;
        wgt[q][2] = ly * hx;
        wgt[q][3] = ly * lx;
      }
    const float count = (float)(G * G);
    const size_t plane_sz = (size_t)L.H * L.W;
    float* out = (depth ? a.out_depth : a.out_rgb) + (size_t)r * C * P * P;
#pragma unroll 4
    for (int c = c0 + wv; c < c0 + kSlab && c < C; c += 4) {
      const float* plane = L.feat + ((size_t)b * C + c) * plane_sz;
      float v[G * G][4];
#pragma unroll
      for (int q = 0; q < G * G; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) v[q][t] = plane[off[q][t]];
      float acc = 0.f;
#pragma unroll
      for (int q = 0; q < G * G; ++q) {
        const float val = ((wgt[q][0] * v[q][0] + wgt[q][1] * v[q][1]) + wgt[q][2] * v[q][2]) + wgt[q][3] * v[q][3];  // :63
        acc = acc + (ok[q] ? val : 0.f);
      }
      out[(size_t)c * P * P + bin_id] = acc / count;
    }
  }
}

// Backward (ROIAlign_cuda.cu:178-262): every output gradient is spread over the 4 taps of each of its G x G
// samples as top_diff * w / count, accumulated into the map gradient with atomic adds (several ROIs and bins
// touch the same pixel).  Same mapping and the same LDS sample table as the forward kernel.
template <int G, bool WALK>
__global__ __launch_bounds__(256) void roi_pool_backward_kernel(RoiPoolArgs a) {
  __shared__ AxisTable ty, tx;
  __shared__ int s_level;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;
  if (tid == 0) {
    int lvl = 0;
    if (a.n_levels > 1) {
      const float area = ((roi[3] - roi[1]) + 1.f) * ((roi[4] - roi[2]) + 1.f);
      const float s = sqrtf(area);
      float t = floorf(4.f + log2f(s / 224.f + 1e-6f));
      t = fminf(fmaxf(t, (float)a.k_min), (float)a.k_max);
      lvl = (int)t - a.k_min;
    }
    s_level = lvl;
  }
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  float* grad_map = depth ? a.depth_grad : a.lv_grad[s_level];
  const int P = a.pooled, n_axis = P * G;
  if (tid < 2 * n_axis) {
    const bool is_y = tid < n_axis;
    const int k = is_y ? tid : tid - n_axis;
    const float lo_c = (is_y ? roi[2] : roi[1]) * L.scale;
    const float hi_c = (is_y ? roi[4] : roi[3]) * L.scale;
    const float len = fmaxf(hi_c - lo_c, 1.0f);
    const float bin = len / (float)P;
    axis_entry(is_y ? ty : tx, k, lo_c, bin, k / G, k % G, G, is_y ? L.H : L.W);
  }
  __syncthreads();
  const int b = (int)roi[0];
  const int wv = tid >> 6;
  const int n_pass = WALK ? (P * P + 63) / 64 : 1;
  for (int pass = 0; pass < n_pass; ++pass) {
    const int bin_id = pass * 64 + (tid & 63);
    const int ph = bin_id / P, pw = bin_id % P;
    if (bin_id >= P * P) return;
    int off[G * G][4];
    float wgt[G * G][4];
    bool ok[G * G];
#pragma unroll
    for (int iy = 0; iy < G; ++iy)
#pragma unroll
      for (int ix = 0; ix < G; ++ix) {
        const int ky = ph * G + iy, kx = pw * G + ix, q = iy * G + ix;
        ok[q] = ty.valid[ky] && tx.valid[kx];
        const float hy = ty.h[ky], ly = ty.l[ky], hx = tx.h[kx], lx = tx.l[kx];
        off[q][0] = ty.lo[ky] * L.W + tx.lo[kx];
        off[q][1] = ty.lo[ky] * L.W + tx.hi[kx];
        off[q][2] = ty.hi[ky] * L.W + tx.lo[kx];
        off[q][3] = ty.hi[ky] * L.W + tx.hi[kx];
        wgt[q][0] = hy * hx;
        wgt[q][1] = hy * lx;
        wgt[q][2] = ly * hx;
        wgt[q][3] = ly * lx;
      }
    const float count = (float)(G * G);
    const size_t plane_sz = (size_t)L.H * L.W;
    const float* gout = (depth ? a.gout_depth : a.gout_rgb) + (size_t)r * C * P * P;
    for (int c = c0 + wv; c < c0 + kSlab && c < C; c += 4) {
      float* plane = grad_map + ((size_t)b * C + c) * plane_sz;
      const float g = gout[(size_t)c * P * P + bin_id];
#pragma unroll
      for (int q = 0; q < G * G; ++q)
        if (ok[q]) {
#pragma unroll
          for (int t = 0; t < 4; ++t) atomicAdd(plane + off[q][t], g * wgt[q][t] / count);   // :240-243
        }
    }
  }
}

// Ordered backward (veto_roi_pool_backward_ordered): the gather that the scatter above inverts, so that every map pixel's sum has ONE
// order -- (ROI, bin row, bin column, sample iy, sample ix, tap), ascending -- whatever the hardware does.  One launch per map.
// Mapping: a workgroup owns a 32 x 8 pixel tile of one image's map and a 32-channel slab; a thread owns one pixel and keeps the slab's 32
// sums in registers.  The workgroup walks the ROIs in index order, 256 at a time: thread i tests ROI i (image, level, footprint against the
// tile), a ballot compacts the hits in order, and the hits' axis tables -- the forward's, built by the same axis_entry -- pass through LDS
// 8 ROIs at a time.  A thread finds the few (ky, kx) entries whose low / high index is its pixel as four bit masks per ROI, then walks
// its own bins in order and adds g * w / count per channel in tap order.  Tiles that no ROI reaches (most of a map) cost the index walk and a store of zeros: the call
// writes every element, which replaces the caller's memset of the atomic form.
constexpr int kTileW = 32, kTileH = 8;
constexpr int kRoiPass = 256;    // ROIs tested per pass, one per thread
constexpr int kRoiStage = 8;     // ROIs whose axis tables are in LDS at once

template <int G>
__global__ __launch_bounds__(256) void roi_pool_backward_ordered_kernel(RoiPoolArgs a, int level, int tiles_x) {   // level < 0: the depth map
  __shared__ AxisTable ty[kRoiStage], tx[kRoiStage];
  __shared__ int s_list[kRoiPass];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool depth = level < 0;
  const RoiLevel L = depth ? a.depth : a.lv[level];
  const int C = depth ? a.depth_channels : a.channels;
  const int b = blockIdx.y, c0 = blockIdx.z * kSlab;
  if (c0 >= C) return;      // (uniform)
  const int tile_x0 = (blockIdx.x % tiles_x) * kTileW, tile_y0 = (blockIdx.x / tiles_x) * kTileH;
  const int x = tile_x0 + (tid & (kTileW - 1)), y = tile_y0 + tid / kTileW;
  const bool live = x < L.W && y < L.H;
  const int P = a.pooled, n_axis = P * G;
  const float count = (float)(G * G);
  const float* gout = depth ? a.gout_depth : a.gout_rgb;
  float acc[kSlab];
#pragma unroll
  for (int c = 0; c < kSlab; ++c) acc[c] = 0.f;

  for (int r0 = 0; r0 < a.n_roi; r0 += kRoiPass) {
    // ---- which ROIs of this pass can touch the tile: a superset (the masks below decide), kept in ROI order
    bool hit = false;
    const int r = r0 + tid;
    if (r < a.n_roi) {
      const float* roi = a.rois + (size_t)r * 5;
      bool mine = (int)roi[0] == b;
      if (mine && !depth && a.n_levels > 1) {      // LevelMapper, as roi_pool_kernel computes it
        const float area = ((roi[3] - roi[1]) + 1.f) * ((roi[4] - roi[2]) + 1.f);
        const float s = sqrtf(area);
        float t = floorf(4.f + log2f(s / 224.f + 1e-6f));
        t = fminf(fmaxf(t, (float)a.k_min), (float)a.k_max);
        mine = (int)t - a.k_min == level;
      }
      if (mine) {
        // a sample coordinate lies in [start, start + len]; its taps in [floor, floor + 1], clamped into the map: one pixel of margin each way
        auto reach = [](float lo_c, float hi_c, int size, int t0, int t1) {
          const float len = fmaxf(hi_c - lo_c, 1.0f);
          const float f0 = fminf(fmaxf(lo_c, 0.f), (float)size), f1 = fminf(fmaxf(lo_c + len, 0.f), (float)size);
          return (int)f0 - 1 <= t1 && (int)f1 + 2 >= t0;
        };
        hit = reach(roi[2] * L.scale, roi[4] * L.scale, L.H, tile_y0, tile_y0 + kTileH - 1) &&
              reach(roi[1] * L.scale, roi[3] * L.scale, L.W, tile_x0, tile_x0 + kTileW - 1);
      }
    }
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) s_cnt[wv] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wv) before += s_cnt[w];
      total += s_cnt[w];
    }
    if (hit) s_list[before + __popcll(votes & ((1ull << lane) - 1ull))] = r;
    __syncthreads();

    for (int i0 = 0; i0 < total; i0 += kRoiStage) {
      const int ns = total - i0 < kRoiStage ? total - i0 : kRoiStage;
      for (int e = tid; e < ns * 2 * n_axis; e += 256) {
        const int j = e / (2 * n_axis), k2 = e % (2 * n_axis);
        const bool is_y = k2 < n_axis;
        const int k = is_y ? k2 : k2 - n_axis;
        const float* roi = a.rois + (size_t)s_list[i0 + j] * 5;
        const float lo_c = (is_y ? roi[2] : roi[1]) * L.scale;
        const float hi_c = (is_y ? roi[4] : roi[3]) * L.scale;
        const float len = fmaxf(hi_c - lo_c, 1.0f);
        const float bin = len / (float)P;
        axis_entry(is_y ? ty[j] : tx[j], k, lo_c, bin, k / G, k % G, G, is_y ? L.H : L.W);
      }
      __syncthreads();
      if (live) {
        for (int j = 0; j < ns; ++j) {
          const AxisTable& Y = ty[j];
          const AxisTable& X = tx[j];
          unsigned ylo = 0, yhi = 0, xlo = 0, xhi = 0;      // bit k: entry k is valid and its low / high index is this pixel's
          for (int k = 0; k < n_axis; ++k) {
            if (Y.valid[k]) { ylo |= (unsigned)(Y.lo[k] == y) << k; yhi |= (unsigned)(Y.hi[k] == y) << k; }
            if (X.valid[k]) { xlo |= (unsigned)(X.lo[k] == x) << k; xhi |= (unsigned)(X.hi[k] == x) << k; }
          }
          const unsigned ya = ylo | yhi, xa = xlo | xhi;
          if (!ya || !xa) continue;
          const float* gr = gout + ((size_t)s_list[i0 + j] * C + c0) * P * P;
          // this lane's bins in (bin row, bin column) order, lowest set bit first: a lane walks only the few bins that touch its pixel (a
          // loop over all P x P bins made every wave walk the union of its lanes' bins: 12.2 against 4.0 ms per call at 12 x 36 boxes)
          constexpr unsigned gm = (1u << G) - 1u;
          for (unsigned yrem = ya; yrem;) {
            const int ph = (__ffs(yrem) - 1) / G;
            yrem &= ~(gm << (ph * G));
            for (unsigned xrem = xa; xrem;) {
              const int pw = (__ffs(xrem) - 1) / G;
              xrem &= ~(gm << (pw * G));
              const float* gb = gr + ph * P + pw;
              float g[kSlab];      // the bin's pooled gradient per channel: shared by its G x G samples
#pragma unroll
              for (int c = 0; c < kSlab; ++c) g[c] = c0 + c < C ? gb[(size_t)c * P * P] : 0.f;      // (uniform condition)
              for (int iy = 0; iy < G; ++iy) {
                const int ky = ph * G + iy;
                if (!((ya >> ky) & 1u)) continue;
                for (int ix = 0; ix < G; ++ix) {
                  const int kx = pw * G + ix;
                  if (!((xa >> kx) & 1u)) continue;
                  const float hy = Y.h[ky], ly = Y.l[ky], hx = X.h[kx], lx = X.l[kx];
                  const float w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;      // :61, the taps of roi_pool_backward_kernel
                  const bool t0 = ((ylo >> ky) & (xlo >> kx) & 1u) != 0, t1 = ((ylo >> ky) & (xhi >> kx) & 1u) != 0;
                  const bool t2 = ((yhi >> ky) & (xlo >> kx) & 1u) != 0, t3 = ((yhi >> ky) & (xhi >> kx) & 1u) != 0;
#pragma unroll
                  for (int c = 0; c < kSlab; ++c) {      // (channels past C add into sums that are never stored)
                    if (t0) acc[c] = acc[c] + g[c] * w0 / count;
                    if (t1) acc[c] = acc[c] + g[c] * w1 / count;
                    if (t2) acc[c] = acc[c] + g[c] * w2 / count;
                    if (t3) acc[c] = acc[c] + g[c] * w3 / count;
                  }
                }
              }
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (live) {
    float* dst = (depth ? a.depth_grad : a.lv_grad[level]) + (((size_t)b * C + c0) * L.H + y) * L.W + x;
    const size_t plane_sz = (size_t)L.H * L.W;
#pragma unroll
    for (int c = 0; c < kSlab; ++c)
      if (c0 + c < C) dst[(size_t)c * plane_sz] = acc[c];
  }
}

// pooled 1..16, sampling ratio 1..4, and an axis table of pooled * sampling_ratio <= kMaxAxis entries (the ordered kernel's bit masks too)
bool roi_pool_sizes_ok(const RoiPoolArgs& a) {
  return a.pooled >= 1 && a.pooled <= 16 && a.sampling_ratio >= 1 && a.sampling_ratio <= 4 && a.pooled * a.sampling_ratio <= kMaxAxis;
}

}  // namespace

hipError_t launch_roi_pool(const RoiPoolArgs& a, hipStream_t s) {
  if (!roi_pool_sizes_ok(a)) return hipErrorInvalidValue;
  const int cmax = a.depth.feat && a.depth_channels > a.channels ? a.depth_channels : a.channels;
  dim3 grid(a.n_roi, (cmax + kSlab - 1) / kSlab, a.depth.feat ? 2 : 1);
  const bool walk = a.pooled > 8;
  switch (a.sampling_ratio) {
    case 1:
      if (walk) VETO_LAUNCH((roi_pool_kernel<1, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<1, false>), grid, dim3(256), 0, s, a);
      break;
    case 2:
      if (walk) VETO_LAUNCH((roi_pool_kernel<2, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<2, false>), grid, dim3(256), 0, s, a);
      break;
    case 3:
      if (walk) VETO_LAUNCH((roi_pool_kernel<3, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<3, false>), grid, dim3(256), 0, s, a);
      break;
    case 4: VETO_LAUNCH((roi_pool_kernel<4, false>), grid, dim3(256), 0, s, a); break;      // (pooled <= 8: 4 x 9 samples would not fit the axis table)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_roi_pool_backward(const RoiPoolArgs& a, hipStream_t s) {
  if (!roi_pool_sizes_ok(a)) return hipErrorInvalidValue;
  const bool with_depth = a.depth.feat && a.gout_depth && a.depth_grad;
  const int cmax = with_depth && a.depth_channels > a.channels ? a.depth_channels : a.channels;
  dim3 grid(a.n_roi, (cmax + kSlab - 1) / kSlab, with_depth ? 2 : 1);
  const bool walk = a.pooled > 8;
  switch (a.sampling_ratio) {
    case 1:
      if (walk) VETO_LAUNCH((roi_pool_backward_kernel<1, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_backward_kernel<1, false>), grid, dim3(256), 0, s, a);
      break;
    case 2:
      if (walk) VETO_LAUNCH((roi_pool_backward_kernel<2, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_backward_kernel<2, false>), grid, dim3(256), 0, s, a);
      break;
    case 3:
      if (walk) VETO_LAUNCH((roi_pool_backward_kernel<3, true>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_backward_kernel<3, false>), grid, dim3(256), 0, s, a);
      break;
    case 4: VETO_LAUNCH((roi_pool_backward_kernel<4, false>), grid, dim3(256), 0, s, a); break;      // (pooled <= 8: 4 x 9 samples would not fit the axis table)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_roi_pool_backward_ordered(const RoiPoolArgs& a, int n_img, hipStream_t s) {
  if (!roi_pool_sizes_ok(a) || n_img < 1 || n_img > 65535) return hipErrorInvalidValue;
  const bool with_depth = a.depth.feat && a.gout_depth && a.depth_grad;
  for (int level = with_depth ? -1 : 0; level < a.n_levels; ++level) {
    const RoiLevel& L = level < 0 ? a.depth : a.lv[level];
    const int C = level < 0 ? a.depth_channels : a.channels;
    const int tiles_x = (L.W + kTileW - 1) / kTileW, tiles_y = (L.H + kTileH - 1) / kTileH;
    dim3 grid((unsigned)tiles_x * tiles_y, n_img, (C + kSlab - 1) / kSlab);
    switch (a.sampling_ratio) {
      case 1: VETO_LAUNCH(roi_pool_backward_ordered_kernel<1>, grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 2: VETO_LAUNCH(roi_pool_backward_ordered_kernel<2>, grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 3: VETO_LAUNCH(roi_pool_backward_ordered_kernel<3>, grid, dim3(256), 0, s, a, level, tiles_x); break;
      default: VETO_LAUNCH(roi_pool_backward_ordered_kernel<4>, grid, dim3(256), 0, s, a, level, tiles_x); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace veto
