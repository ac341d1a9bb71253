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
// Map forms: the above is the NCHW mapping, instantiated on the maps' element type (float32, float16, bfloat16; a load widens to
// float32).  NHWC maps (torch.channels_last) have kernels of their own further down, with the lanes over channels.
// The adaptive grid (sampling ratio 0: the grid chosen per ROI) has NCHW kernels of its own at the end, without axis tables.
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

// one axis entry, ROIAlign_cuda.cu:21-57 restricted to one coordinate: the coordinate of sample i of bin p on a grid of `grid`
// samples per bin (non-decreasing in i: every operation is a monotone rounding of a monotone function), ...
__device__ __forceinline__ float axis_coord(float start, float bin, int p, int i, int grid) {
  return (start + (float)p * bin) + (((float)i + 0.5f) * bin) / (float)grid;
}

// ... and its validity, tap indices and low weight
struct AxisTap {
  int lo, hi;
  float l;
  bool valid;
};
__device__ __forceinline__ AxisTap axis_tap(float v, int size) {
  AxisTap e;
  e.valid = !(v < -1.0f || v > (float)size);
  if (v <= 0.f) v = 0.f;
  int lo = (int)v, hi;
  if (lo >= size - 1) {
    hi = lo = size - 1;
    v = (float)lo;
  } else {
    hi = lo + 1;
  }
  e.lo = lo;
  e.hi = hi;
  e.l = v - (float)lo;
  return e;
}

__device__ __forceinline__ void axis_entry(AxisTable& t, int k, float start, float bin, int p, int i, int grid, int size) {
  const AxisTap e = axis_tap(axis_coord(start, bin, p, i, grid), size);
  t.lo[k] = e.valid ? e.lo : 0;
  t.hi[k] = e.valid ? e.hi : 0;
  t.l[k] = e.l;
  t.h[k] = 1.0f - e.l;
  t.valid[k] = e.valid;
}

// LevelMapper: floor(4 + log2(sqrt(area) / 224 + 1e-6)) clamped to [k_min, k_max], minus k_min; the
// area uses the +1 pixel convention of BoxList.area() (bounding_box.py:249-259).  One level: 0.
__device__ __forceinline__ int roi_level(const RoiPoolArgs& a, const float* roi) {
  if (a.n_levels <= 1) return 0;
  const float area = ((roi[3] - roi[1]) + 1.f) * ((roi[4] - roi[2]) + 1.f);
  const float s = sqrtf(area);
  float t = floorf(4.f + log2f(s / 224.f + 1e-6f));
  t = fminf(fmaxf(t, (float)a.k_min), (float)a.k_max);
  return (int)t - a.k_min;
}

// entry k2 of an ROI's two axis tables (0 .. P * G - 1: the y axis, then the x axis) on the map L
__device__ __forceinline__ void roi_axis_pair_entry(AxisTable& ty, AxisTable& tx, const float* roi, const RoiLevel& L, int P, int G, int k2) {
  const int n_axis = P * G;
  const bool is_y = k2 < n_axis;
  const int k = is_y ? k2 : k2 - n_axis;
  // :84-98 no rounding of the scaled box; malformed ROIs become 1x1
  const float lo_c = (is_y ? roi[2] : roi[1]) * L.scale;
  const float hi_c = (is_y ? roi[4] : roi[3]) * L.scale;
  const float len = fmaxf(hi_c - lo_c, 1.0f);
  const float bin = len / (float)P;
  axis_entry(is_y ? ty : tx, k, lo_c, bin, k / G, k % G, G, is_y ? L.H : L.W);
}

// The element types a map may have (RoiDtype).  A load widens to float32, which is exact for both 16-bit types: everything
// after the load is the float32 arithmetic.
struct bf16_t { unsigned short bits; };
__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(_Float16 v) { return (float)v; }
__device__ __forceinline__ float widen(bf16_t v) { return __uint_as_float((unsigned)v.bits << 16); }

template <int G, bool WALK, typename T>  // G = sampling ratio (samples per bin and axis); WALK: pooled > 8, a lane owns several bins; T: the maps' element type
__global__ __launch_bounds__(256) void roi_pool_kernel(RoiPoolArgs a) {
  __shared__ AxisTable ty, tx;
  __shared__ int s_level;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;

  if (tid == 0) {
    const int lvl = roi_level(a, roi);
    s_level = lvl;
    if (a.out_levels && !depth && blockIdx.y == 0) a.out_levels[r] = lvl;
  }
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  const int P = a.pooled, n_axis = P * G;
  if (tid < 2 * n_axis) roi_axis_pair_entry(ty, tx, roi, L, P, G, tid);
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
    // four channel planes in flight; a 16-bit map at 4 x 4 samples one: its 64 taps take an address pair each (the compiler forms no
    // base + 32-bit offset load for them), and four planes of those spilled 668 bytes per lane
    constexpr int kPlanes = sizeof(T) == 4 || G < 4 ? 4 : 1;
#pragma unroll kPlanes
    for (int c = c0 + wv; c < c0 + kSlab && c < C; c += 4) {
      const T* plane = (const T*)L.feat + ((size_t)b * C + c) * plane_sz;
      float v[G * G][4];
#pragma unroll
      for (int q = 0; q < G * G; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) v[q][t] = widen(plane[off[q][t]]);
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
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;
  if (tid == 0) s_level = roi_level(a, roi);
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  float* grad_map = depth ? a.depth_grad : a.lv_grad[s_level];
  const int P = a.pooled, n_axis = P * G;
  if (tid < 2 * n_axis) roi_axis_pair_entry(ty, tx, roi, L, P, G, tid);
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

template <int G, bool NHWC>      // NHWC: the gradient map is [n_img, H, W, C]; the sums and their order are the same
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
      if (mine && !depth && a.n_levels > 1) mine = roi_level(a, roi) == level;      // LevelMapper, as roi_pool_kernel computes it
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
        roi_axis_pair_entry(ty[j], tx[j], a.rois + (size_t)s_list[i0 + j] * 5, L, P, G, k2);
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
    float* base = depth ? a.depth_grad : a.lv_grad[level];
    if constexpr (NHWC) {
      // the pixel's slab is 32 contiguous floats.  c0 is a multiple of 32, so with C a multiple of 4 and a 16-byte aligned map every
      // group of four is aligned and lies wholly inside or wholly outside the C channels; otherwise element by element
      float* dst = base + (((size_t)b * L.H + y) * L.W + x) * C + c0;
      if ((C & 3) == 0 && ((uintptr_t)base & 15) == 0) {
#pragma unroll
        for (int c = 0; c < kSlab; c += 4)
          if (c0 + c < C) *reinterpret_cast<float4*>(dst + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
      } else {
#pragma unroll
        for (int c = 0; c < kSlab; ++c)
          if (c0 + c < C) dst[c] = acc[c];
      }
    } else {
      float* dst = base + (((size_t)b * C + c0) * L.H + y) * L.W + x;
      const size_t plane_sz = (size_t)L.H * L.W;
#pragma unroll
      for (int c = 0; c < kSlab; ++c)
        if (c0 + c < C) dst[(size_t)c * plane_sz] = acc[c];
    }
  }
}

// ---- NHWC maps ([n_img, H, W, C], torch.channels_last) ----------------------------------------------------------------------------------
// One tap of one bin is a contiguous channel vector, so the lanes of a wave are 64 consecutive channels: a tap is one full-line
// load (forward; four channels per lane where alignment allows, see load_channels) or one run of 256 contiguous bytes of float
// atomics (backward), and its offsets and weights are wave-uniform reads of the LDS axis tables.  One workgroup per (ROI, 64-channel slab); wave w takes the bins w, w + 4, ... of a pass of 64 bins.
// The pooled tensors stay [n_roi, C, P, P]: a 64-channel x 64-bin float32 tile (padded rows, 16.25 KiB) is transposed through LDS so
// that the global side is contiguous 256-byte rows there too.  The sampling ratio is a run-time loop here: nothing per lane depends
// on it.  Same axis tables, level choice and operation order as the NCHW kernels above.
constexpr int kSlabN = 64;

// V consecutive channels of one pixel, widened.  V = 4 is one 16-byte (float32) or 8-byte (16-bit) load and needs that alignment:
// the launcher takes it only where the channel count is a multiple of 4 and every map of the launch starts on such a boundary.
template <int V, typename T>
__device__ __forceinline__ void load_channels(const T* p, float (&v)[V]) {
  if constexpr (V == 1) {
    v[0] = widen(p[0]);
  } else if constexpr (sizeof(T) == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    T e[4];
    __builtin_memcpy(e, &q, 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = widen(e[i]);
  }
}

template <typename T, int V>      // V channels per lane: 1 (any map) or 4 (vector loads)
__global__ __launch_bounds__(256) void roi_pool_nhwc_kernel(RoiPoolArgs a) {
  __shared__ AxisTable ty, tx;
  __shared__ int s_level;
  __shared__ float tile[kSlabN][65];
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlabN;
  if (c0 >= C) return;
  if (tid == 0) {
    const int lvl = roi_level(a, roi);
    s_level = lvl;
    if (a.out_levels && !depth && blockIdx.y == 0) a.out_levels[r] = lvl;
  }
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  const int P = a.pooled, G = a.sampling_ratio;
  if (tid < 2 * P * G) roi_axis_pair_entry(ty, tx, roi, L, P, G, tid);
  __syncthreads();

  // kLanes lanes cover the slab's channels, V each; the workgroup works on kSlots bins at a time (V = 1: a wave per bin, the tap
  // offsets wave-uniform; V = 4: sixteen lanes per bin, four bins per wave)
  constexpr int kLanes = kSlabN / V, kSlots = 256 / kLanes;
  const int b = (int)roi[0];
  const int lane = tid & 63, wv = tid >> 6;
  const int cl = tid % kLanes, slot = tid / kLanes;
  const int c = c0 + cl * V;      // (V = 4: C is a multiple of 4, so c < C covers c .. c + 3)
  const float count = (float)(G * G);
  const T* img = (const T*)L.feat + (size_t)b * L.H * L.W * C;
  float* out = (depth ? a.out_depth : a.out_rgb) + (size_t)r * C * P * P;
  for (int bin0 = 0; bin0 < P * P; bin0 += 64) {
    for (int j = slot; j < 64; j += kSlots) {
      const int bin_id = bin0 + j;
      if (bin_id >= P * P) break;
      const int ph = bin_id / P, pw = bin_id % P;
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; ++i) acc[i] = 0.f;
      if (c < C) {
        for (int iy = 0; iy < G; ++iy)
          for (int ix = 0; ix < G; ++ix) {
            const int ky = ph * G + iy, kx = pw * G + ix;
            if (!(ty.valid[ky] && tx.valid[kx])) continue;      // bilinear_interpolate returns 0 (:26-29); acc + 0 is acc (a sum from +0 never holds -0)
            const float hy = ty.h[ky], ly = ty.l[ky], hx = tx.h[kx], lx = tx.l[kx];
            const float w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;      // :61
            const size_t row_lo = (size_t)ty.lo[ky] * L.W, row_hi = (size_t)ty.hi[ky] * L.W;
            float v0[V], v1[V], v2[V], v3[V];
            load_channels<V>(img + (row_lo + tx.lo[kx]) * C + c, v0);
            load_channels<V>(img + (row_lo + tx.hi[kx]) * C + c, v1);
            load_channels<V>(img + (row_hi + tx.lo[kx]) * C + c, v2);
            load_channels<V>(img + (row_hi + tx.hi[kx]) * C + c, v3);
#pragma unroll
            for (int i = 0; i < V; ++i) {
              const float val = ((w0 * v0[i] + w1 * v1[i]) + w2 * v2[i]) + w3 * v3[i];      // :63
              acc[i] = acc[i] + val;
            }
          }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) tile[cl * V + i][j] = acc[i] / count;
    }
    __syncthreads();
    for (int cc = wv; cc < kSlabN; cc += 4)
      if (c0 + cc < C && bin0 + lane < P * P) out[(size_t)(c0 + cc) * P * P + bin0 + lane] = tile[cc][lane];
    __syncthreads();
  }
}

// the atomic backward into NHWC gradient maps: the pooled gradients pass through the same LDS tile the other way
__global__ __launch_bounds__(256) void roi_pool_backward_nhwc_kernel(RoiPoolArgs a) {
  __shared__ AxisTable ty, tx;
  __shared__ int s_level;
  __shared__ float tile[kSlabN][65];
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlabN;
  if (c0 >= C) return;
  if (tid == 0) s_level = roi_level(a, roi);
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  const int P = a.pooled, G = a.sampling_ratio;
  if (tid < 2 * P * G) roi_axis_pair_entry(ty, tx, roi, L, P, G, tid);
  __syncthreads();

  const int b = (int)roi[0];
  const int lane = tid & 63, wv = tid >> 6;
  const int c = c0 + lane;
  const float count = (float)(G * G);
  float* img = (depth ? a.depth_grad : a.lv_grad[s_level]) + (size_t)b * L.H * L.W * C;
  const float* gout = (depth ? a.gout_depth : a.gout_rgb) + (size_t)r * C * P * P;
  for (int bin0 = 0; bin0 < P * P; bin0 += 64) {
    for (int cc = wv; cc < kSlabN; cc += 4)
      tile[cc][lane] = c0 + cc < C && bin0 + lane < P * P ? gout[(size_t)(c0 + cc) * P * P + bin0 + lane] : 0.f;
    __syncthreads();
    for (int j = wv; j < 64; j += 4) {
      const int bin_id = bin0 + j;
      if (bin_id >= P * P) break;      // (wave-uniform)
      if (c >= C) continue;
      const int ph = bin_id / P, pw = bin_id % P;
      const float g = tile[lane][j];
      for (int iy = 0; iy < G; ++iy)
        for (int ix = 0; ix < G; ++ix) {
          const int ky = ph * G + iy, kx = pw * G + ix;
          if (!(ty.valid[ky] && tx.valid[kx])) continue;
          const float hy = ty.h[ky], ly = ty.l[ky], hx = tx.h[kx], lx = tx.l[kx];
          const size_t row_lo = (size_t)ty.lo[ky] * L.W, row_hi = (size_t)ty.hi[ky] * L.W;
          atomicAdd(img + (row_lo + tx.lo[kx]) * C + c, g * (hy * hx) / count);      // :240-243, the taps in the NCHW kernel's order
          atomicAdd(img + (row_lo + tx.hi[kx]) * C + c, g * (hy * lx) / count);
          atomicAdd(img + (row_hi + tx.lo[kx]) * C + c, g * (ly * hx) / count);
          atomicAdd(img + (row_hi + tx.hi[kx]) * C + c, g * (ly * lx) / count);
        }
    }
    __syncthreads();
  }
}

// ---- the adaptive sampling grid (sampling_ratio == 0, ROIAlign_cuda.cu:103-104) -----------------------------------------------------------
// The grid is chosen per ROI and axis: g = ceil(len / P) samples per bin, from the float32 quotient.  Same mapping as roi_pool_kernel
// (a workgroup per (ROI, 32-channel slab), the lanes are bins, a lane walks bins lane, lane + 64, ... for P > 8, the four waves
// take channel planes), but there is no axis table: g has no bound a table could be sized for, so every entry is computed where it
// is used, by the axis_coord / axis_tap that axis_entry is made of -- once per sample, then used for the wave's kSlab / 4 channels,
// which have an accumulator each in registers.  One bin's sum is never split: iy outer, ix inner, sequential, as in the reference.
//
// Work bound.  axis_coord is non-decreasing in i, so the valid samples of an axis of a bin are ONE index range; axis_first finds its
// two ends by bisection on the same float32 expression (at most 31 steps each) and the loops run over the product of the two ranges.
// The spacing bin / g is in (0.5, 1] once len >= P (below that g = 1), so an axis has at most 2 * size + 3 valid samples whatever
// the box: a ROI of +-4000 px costs what its part inside the map costs.  A range longer than that can only come from coordinates
// that float32 no longer separates (or from NaN, which every comparison lets through); it is outside the contract and taken as empty.
struct AdaptiveAxis {
  float start, bin;
  int g;
};

__device__ __forceinline__ AdaptiveAxis adaptive_axis(float lo, float hi, float scale, int P) {
  const float lo_c = lo * scale, hi_c = hi * scale;
  const float len = fmaxf(hi_c - lo_c, 1.0f);      // :95-96
  AdaptiveAxis A;
  A.start = lo_c;
  A.bin = len / (float)P;
  A.g = (int)fminf(ceilf(len / (float)P), 2147483520.f);      // :103-104; the clamp keeps the conversion defined for an infinite box
  return A;
}

// the first i in [0, g] whose coordinate is > size (UPPER) or no longer < -1 (!UPPER); g when there is none
template <bool UPPER>
__device__ __forceinline__ int axis_first(const AdaptiveAxis& A, int p, int size) {
  int lo = 0, hi = A.g;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const float v = axis_coord(A.start, A.bin, p, mid, A.g);
    if (UPPER ? v > (float)size : !(v < -1.0f)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// [i0, i0 + n): the valid samples of bin p on this axis
__device__ __forceinline__ void axis_valid_range(const AdaptiveAxis& A, int p, int size, int& i0, int& n) {
  i0 = n = 0;
  if (!(fabsf(A.start) <= 3.0e38f && A.bin <= 3.0e38f)) return;      // NaN or infinite box: no comparison would hold a NaN sample back
  i0 = axis_first<false>(A, p, size);
  n = axis_first<true>(A, p, size) - i0;
  if (n < 0 || n > 2 * size + 3) n = 0;
}

constexpr int kPerWave = kSlab / 4;      // channels of a slab that one wave takes: c0 + wave, + 4, ...

template <typename T>
__global__ __launch_bounds__(256) void roi_pool_adaptive_kernel(RoiPoolArgs a) {
  __shared__ int s_level;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;
  if (tid == 0) {
    const int lvl = roi_level(a, roi);
    s_level = lvl;
    if (a.out_levels && !depth && blockIdx.y == 0) a.out_levels[r] = lvl;
  }
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  const int P = a.pooled;
  const AdaptiveAxis ay = adaptive_axis(roi[2], roi[4], L.scale, P), ax = adaptive_axis(roi[1], roi[3], L.scale, P);
  const float count = (float)(int)((unsigned)ay.g * (unsigned)ax.g);      // :112 (an int product in the reference)
  const int b = (int)roi[0];
  const int wv = tid >> 6;
  const size_t plane_sz = (size_t)L.H * L.W;
  const T* base = (const T*)L.feat + ((size_t)b * C + c0 + wv) * plane_sz;
  float* out = (depth ? a.out_depth : a.out_rgb) + ((size_t)r * C + c0 + wv) * P * P;
  const int n_pass = (P * P + 63) / 64;
  for (int pass = 0; pass < n_pass; ++pass) {
    const int bin_id = pass * 64 + (tid & 63);
    if (bin_id >= P * P) return;
    const int ph = bin_id / P, pw = bin_id % P;
    int y0, ny, x0, nx;
    axis_valid_range(ay, ph, L.H, y0, ny);
    axis_valid_range(ax, pw, L.W, x0, nx);
    float acc[kPerWave];
#pragma unroll
    for (int j = 0; j < kPerWave; ++j) acc[j] = 0.f;
    for (int iy = y0; iy < y0 + ny; ++iy) {
      const AxisTap ey = axis_tap(axis_coord(ay.start, ay.bin, ph, iy, ay.g), L.H);
      const float ly = ey.l, hy = 1.0f - ey.l;
      for (int ix = x0; ix < x0 + nx; ++ix) {
        const AxisTap ex = axis_tap(axis_coord(ax.start, ax.bin, pw, ix, ax.g), L.W);
        const float lx = ex.l, hx = 1.0f - ex.l;
        const float w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;      // :61
        const int o0 = ey.lo * L.W + ex.lo, o1 = ey.lo * L.W + ex.hi, o2 = ey.hi * L.W + ex.lo, o3 = ey.hi * L.W + ex.hi;
#pragma unroll
        for (int j = 0; j < kPerWave; ++j)
          if (c0 + wv + 4 * j < C) {      // (wave-uniform)
            const T* plane = base + (size_t)(4 * j) * plane_sz;
            const float v0 = widen(plane[o0]), v1 = widen(plane[o1]), v2 = widen(plane[o2]), v3 = widen(plane[o3]);
            acc[j] = acc[j] + (((w0 * v0 + w1 * v1) + w2 * v2) + w3 * v3);      // :63, :115
          }
      }
    }
    const bool skipped = ny != ay.g || nx != ax.g;      // a sample outside the map adds +0 (:26-29): once is as good as every time
#pragma unroll
    for (int j = 0; j < kPerWave; ++j)
      if (c0 + wv + 4 * j < C) {
        if (skipped) acc[j] = acc[j] + 0.f;
        out[(size_t)(4 * j) * P * P + bin_id] = acc[j] / count;      // :118
      }
  }
}

// Backward on the adaptive grid: the same ranges and the same mapping; per valid sample and tap one atomic add of (g * w) / count,
// the terms of roi_pool_backward_kernel.
__global__ __launch_bounds__(256) void roi_pool_adaptive_backward_kernel(RoiPoolArgs a) {
  __shared__ int s_level;
  const int r = blockIdx.x, tid = threadIdx.x;
  const bool depth = blockIdx.z + a.z0 == 1;
  const float* roi = a.rois + (size_t)r * 5;
  const int C = depth ? a.depth_channels : a.channels;
  const int c0 = blockIdx.y * kSlab;
  if (c0 >= C) return;
  if (tid == 0) s_level = roi_level(a, roi);
  __syncthreads();
  const RoiLevel L = depth ? a.depth : a.lv[s_level];
  float* grad_map = depth ? a.depth_grad : a.lv_grad[s_level];
  const int P = a.pooled;
  const AdaptiveAxis ay = adaptive_axis(roi[2], roi[4], L.scale, P), ax = adaptive_axis(roi[1], roi[3], L.scale, P);
  const float count = (float)(int)((unsigned)ay.g * (unsigned)ax.g);
  const int b = (int)roi[0];
  const int wv = tid >> 6;
  const size_t plane_sz = (size_t)L.H * L.W;
  float* base = grad_map + ((size_t)b * C + c0 + wv) * plane_sz;
  const float* gout = (depth ? a.gout_depth : a.gout_rgb) + ((size_t)r * C + c0 + wv) * P * P;
  const int n_pass = (P * P + 63) / 64;
  for (int pass = 0; pass < n_pass; ++pass) {
    const int bin_id = pass * 64 + (tid & 63);
    if (bin_id >= P * P) return;
    const int ph = bin_id / P, pw = bin_id % P;
    int y0, ny, x0, nx;
    axis_valid_range(ay, ph, L.H, y0, ny);
    axis_valid_range(ax, pw, L.W, x0, nx);
    if (ny == 0 || nx == 0) continue;
    float g[kPerWave];
#pragma unroll
    for (int j = 0; j < kPerWave; ++j) g[j] = c0 + wv + 4 * j < C ? gout[(size_t)(4 * j) * P * P + bin_id] : 0.f;
    for (int iy = y0; iy < y0 + ny; ++iy) {
      const AxisTap ey = axis_tap(axis_coord(ay.start, ay.bin, ph, iy, ay.g), L.H);
      const float ly = ey.l, hy = 1.0f - ey.l;
      for (int ix = x0; ix < x0 + nx; ++ix) {
        const AxisTap ex = axis_tap(axis_coord(ax.start, ax.bin, pw, ix, ax.g), L.W);
        const float lx = ex.l, hx = 1.0f - ex.l;
        const float w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;
        const int o0 = ey.lo * L.W + ex.lo, o1 = ey.lo * L.W + ex.hi, o2 = ey.hi * L.W + ex.lo, o3 = ey.hi * L.W + ex.hi;
#pragma unroll
        for (int j = 0; j < kPerWave; ++j)
          if (c0 + wv + 4 * j < C) {      // (wave-uniform)
            float* plane = base + (size_t)(4 * j) * plane_sz;
            atomicAdd(plane + o0, g[j] * w0 / count);      // :240-243
            atomicAdd(plane + o1, g[j] * w1 / count);
            atomicAdd(plane + o2, g[j] * w2 / count);
            atomicAdd(plane + o3, g[j] * w3 / count);
          }
      }
    }
  }
}

template <typename T>
hipError_t launch_roi_pool_adaptive_group(const RoiPoolArgs& a, int cmax, int nz, hipStream_t s) {
  VETO_LAUNCH((roi_pool_adaptive_kernel<T>), dim3(a.n_roi, (cmax + kSlab - 1) / kSlab, nz), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_roi_pool_adaptive_typed(const RoiPoolArgs& a, int dtype, int cmax, int nz, hipStream_t s) {
  switch (dtype) {
    case kRoiF32: return launch_roi_pool_adaptive_group<float>(a, cmax, nz, s);
    case kRoiF16: return launch_roi_pool_adaptive_group<_Float16>(a, cmax, nz, s);
    case kRoiBF16: return launch_roi_pool_adaptive_group<bf16_t>(a, cmax, nz, s);
    default: return hipErrorInvalidValue;
  }
}

bool roi_pool_adaptive_ok(const RoiPoolArgs& a) {
  return a.pooled >= 1 && a.pooled <= 16 && a.sampling_ratio == 0 && a.lv_layout == kRoiNCHW && a.depth_layout == kRoiNCHW;
}

// pooled 1..16, sampling ratio 1..4, and an axis table of pooled * sampling_ratio <= kMaxAxis entries (the ordered kernel's bit masks too)
bool roi_pool_sizes_ok(const RoiPoolArgs& a) {
  return a.pooled >= 1 && a.pooled <= 16 && a.sampling_ratio >= 1 && a.sampling_ratio <= 4 && a.pooled * a.sampling_ratio <= kMaxAxis;
}

// one forward launch over nz map groups (z0 = 0: the pyramid first; z0 = 1: the depth map alone) that share an element type and a layout
template <typename T>
hipError_t launch_roi_pool_group(const RoiPoolArgs& a, int layout, int cmax, int nz, hipStream_t s) {
  if (layout == kRoiNHWC) {
    // four channels per load where every pixel's channel vector of every map of this launch starts on a 4-element boundary
    const bool levels = a.z0 == 0, with_depth = a.z0 == 1 || nz == 2;
    uintptr_t bits = 0;
    if (levels) {
      bits |= (uintptr_t)a.channels * sizeof(T);
      for (int l = 0; l < a.n_levels; ++l) bits |= (uintptr_t)a.lv[l].feat;
    }
    if (with_depth) bits |= (uintptr_t)a.depth_channels * sizeof(T) | (uintptr_t)a.depth.feat;
    dim3 grid(a.n_roi, (cmax + kSlabN - 1) / kSlabN, nz);
    if ((bits & (4 * sizeof(T) - 1)) == 0) VETO_LAUNCH((roi_pool_nhwc_kernel<T, 4>), grid, dim3(256), 0, s, a);
    else VETO_LAUNCH((roi_pool_nhwc_kernel<T, 1>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
  }
  dim3 grid(a.n_roi, (cmax + kSlab - 1) / kSlab, nz);
  const bool walk = a.pooled > 8;
  switch (a.sampling_ratio) {
    case 1:
      if (walk) VETO_LAUNCH((roi_pool_kernel<1, true, T>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<1, false, T>), grid, dim3(256), 0, s, a);
      break;
    case 2:
      if (walk) VETO_LAUNCH((roi_pool_kernel<2, true, T>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<2, false, T>), grid, dim3(256), 0, s, a);
      break;
    case 3:
      if (walk) VETO_LAUNCH((roi_pool_kernel<3, true, T>), grid, dim3(256), 0, s, a);
      else VETO_LAUNCH((roi_pool_kernel<3, false, T>), grid, dim3(256), 0, s, a);
      break;
    case 4: VETO_LAUNCH((roi_pool_kernel<4, false, T>), grid, dim3(256), 0, s, a); break;      // (pooled <= 8: 4 x 9 samples would not fit the axis table)
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_roi_pool_typed(const RoiPoolArgs& a, int dtype, int layout, int cmax, int nz, hipStream_t s) {
  switch (dtype) {
    case kRoiF32: return launch_roi_pool_group<float>(a, layout, cmax, nz, s);
    case kRoiF16: return launch_roi_pool_group<_Float16>(a, layout, cmax, nz, s);
    case kRoiBF16: return launch_roi_pool_group<bf16_t>(a, layout, cmax, nz, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_roi_pool_backward_group(const RoiPoolArgs& a, int layout, int cmax, int nz, hipStream_t s) {
  if (layout == kRoiNHWC) {
    VETO_LAUNCH(roi_pool_backward_nhwc_kernel, dim3(a.n_roi, (cmax + kSlabN - 1) / kSlabN, nz), dim3(256), 0, s, a);
    return hipGetLastError();
  }
  dim3 grid(a.n_roi, (cmax + kSlab - 1) / kSlab, nz);
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

}  // namespace

// The pyramid and the depth map share one launch (blockIdx.z) when they have one element type and one layout -- always so for
// float32 NCHW maps; otherwise each map group gets the launch of its own form.
hipError_t launch_roi_pool(const RoiPoolArgs& a0, hipStream_t s) {
  if (!roi_pool_sizes_ok(a0)) return hipErrorInvalidValue;
  RoiPoolArgs a = a0;
  const bool with_depth = a.depth.feat != nullptr;
  if (!with_depth || (a.lv_dtype == a.depth_dtype && a.lv_layout == a.depth_layout)) {
    const int cmax = with_depth && a.depth_channels > a.channels ? a.depth_channels : a.channels;
    a.z0 = 0;
    return launch_roi_pool_typed(a, a.lv_dtype, a.lv_layout, cmax, with_depth ? 2 : 1, s);
  }
  a.z0 = 0;
  hipError_t e = launch_roi_pool_typed(a, a.lv_dtype, a.lv_layout, a.channels, 1, s);
  if (e != hipSuccess) return e;
  a.z0 = 1;
  return launch_roi_pool_typed(a, a.depth_dtype, a.depth_layout, a.depth_channels, 1, s);
}

hipError_t launch_roi_pool_backward(const RoiPoolArgs& a0, hipStream_t s) {
  if (!roi_pool_sizes_ok(a0)) return hipErrorInvalidValue;
  RoiPoolArgs a = a0;
  const bool with_depth = a.depth.feat && a.gout_depth && a.depth_grad;
  if (!with_depth || a.lv_layout == a.depth_layout) {
    const int cmax = with_depth && a.depth_channels > a.channels ? a.depth_channels : a.channels;
    a.z0 = 0;
    return launch_roi_pool_backward_group(a, a.lv_layout, cmax, with_depth ? 2 : 1, s);
  }
  a.z0 = 0;
  hipError_t e = launch_roi_pool_backward_group(a, a.lv_layout, a.channels, 1, s);
  if (e != hipSuccess) return e;
  a.z0 = 1;
  return launch_roi_pool_backward_group(a, a.depth_layout, a.depth_channels, 1, s);
}

// The adaptive grid: NCHW maps; one launch when the pyramid and the depth map share an element type, else one each.
hipError_t launch_roi_pool_adaptive(const RoiPoolArgs& a0, hipStream_t s) {
  if (!roi_pool_adaptive_ok(a0)) return hipErrorInvalidValue;
  RoiPoolArgs a = a0;
  const bool with_depth = a.depth.feat != nullptr;
  a.z0 = 0;
  if (!with_depth || a.lv_dtype == a.depth_dtype) {
    const int cmax = with_depth && a.depth_channels > a.channels ? a.depth_channels : a.channels;
    return launch_roi_pool_adaptive_typed(a, a.lv_dtype, cmax, with_depth ? 2 : 1, s);
  }
  hipError_t e = launch_roi_pool_adaptive_typed(a, a.lv_dtype, a.channels, 1, s);
  if (e != hipSuccess) return e;
  a.z0 = 1;
  return launch_roi_pool_adaptive_typed(a, a.depth_dtype, a.depth_channels, 1, s);
}

hipError_t launch_roi_pool_adaptive_backward(const RoiPoolArgs& a0, hipStream_t s) {
  if (!roi_pool_adaptive_ok(a0)) return hipErrorInvalidValue;
  RoiPoolArgs a = a0;
  const bool with_depth = a.depth.feat && a.gout_depth && a.depth_grad;
  const int cmax = with_depth && a.depth_channels > a.channels ? a.depth_channels : a.channels;
  a.z0 = 0;
  VETO_LAUNCH(roi_pool_adaptive_backward_kernel, dim3(a.n_roi, (cmax + kSlab - 1) / kSlab, with_depth ? 2 : 1), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_roi_pool_backward_ordered(const RoiPoolArgs& a, int n_img, hipStream_t s) {
  if (!roi_pool_sizes_ok(a) || n_img < 1 || n_img > 65535) return hipErrorInvalidValue;
  const bool with_depth = a.depth.feat && a.gout_depth && a.depth_grad;
  for (int level = with_depth ? -1 : 0; level < a.n_levels; ++level) {
    const RoiLevel& L = level < 0 ? a.depth : a.lv[level];
    const int C = level < 0 ? a.depth_channels : a.channels;
    const bool nhwc = (level < 0 ? a.depth_layout : a.lv_layout) == kRoiNHWC;
    const int tiles_x = (L.W + kTileW - 1) / kTileW, tiles_y = (L.H + kTileH - 1) / kTileH;
    dim3 grid((unsigned)tiles_x * tiles_y, n_img, (C + kSlab - 1) / kSlab);
    switch (a.sampling_ratio * 2 + (nhwc ? 1 : 0)) {
      case 2: VETO_LAUNCH((roi_pool_backward_ordered_kernel<1, false>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 3: VETO_LAUNCH((roi_pool_backward_ordered_kernel<1, true>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 4: VETO_LAUNCH((roi_pool_backward_ordered_kernel<2, false>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 5: VETO_LAUNCH((roi_pool_backward_ordered_kernel<2, true>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 6: VETO_LAUNCH((roi_pool_backward_ordered_kernel<3, false>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 7: VETO_LAUNCH((roi_pool_backward_ordered_kernel<3, true>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      case 8: VETO_LAUNCH((roi_pool_backward_ordered_kernel<4, false>), grid, dim3(256), 0, s, a, level, tiles_x); break;
      default: VETO_LAUNCH((roi_pool_backward_ordered_kernel<4, true>), grid, dim3(256), 0, s, a, level, tiles_x); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace veto
