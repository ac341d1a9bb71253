// Detection (box mAP) evaluator on the device: the "bbox" branch of do_vg_evaluation
// (pysgg/data/datasets/evaluation/vg/vg_eval.py:67-182), i.e. pycocotools' COCOeval.evaluate() / accumulate() / summarize() as
// that code drives them: iouType 'bbox', no crowd boxes, ten IoU thresholds, 101 recall thresholds, maxDets [1, 10, 100], four
// area ranges, categories 1 .. C-1.  include/veto_amd.h states the arithmetic and the record layout.
//
// Limits (checked by the ABI before any launch): 1024 GT boxes and 1024 detections per image (kMaxGt, kMaxDet: one workgroup
// sorts an image's boxes in LDS), 2..1024 classes (10 bits of the sort keys), fewer than 2^31 records.  Scores are finite as a
// precondition: the score key orders NaNs by their bits, which no numpy sort does.
//
// match (one workgroup per image): sorts the image's detections by (class, score descending, index) and its GT boxes by
// (class, index), runs COCOeval's greedy matching once per (class, threshold, area) -- a thread per combination, the "GT taken"
// flags in the workspace -- at the cut of 100 per (image, class) (the first m detections' matches do not depend on the later
// ones, so accumulate takes prefixes by rank), and writes one record per detection.
// accumulate: an LSD radix sort (8 bits a pass, 6 passes over the 42-bit key, index payload; per pass a tile histogram, one
// scan over [digit][tile] and a stable scatter), the class boundaries, one workgroup per (class, area, maxDets) that scans the
// class segment in chunks of kChunk with a carry, and the twelve stats.
//
// Measured up to 400 000 records only.  Each radix pass scans its whole [256][tiles] histogram with ONE workgroup
// (det_eval_sort_scan_kernel): 256 * ceil(n / 2048) entries, serial in steps of 1024.  That is 50 176 entries a pass at 400 000
// records and about 2.7e8 at the limit of 2^31, so beyond a few million records finalize time is unmeasured and dominated by
// this scan; a split of that size wants a hierarchical scan (tile sums, scan of the sums, add) in its place.
#include "common.h"
#include "kernels.h"
#include "selection.h"

// every comparison below is against numpy's / maskApi.c's separately rounded arithmetic: no FMA contraction
#pragma clang fp contract(off)

namespace veto {

namespace {

constexpr int kMaxDet = 1024, kMaxGt = 1024;
constexpr int kCut = 100;                  // maxDets[-1]: detections kept per (image, class)
constexpr int kT = kDetEvalThrs, kA = kDetEvalAreas, kTA = kT * kA, kR = kDetEvalRecThrs;
constexpr int kThreads = 256;
constexpr int kChunk = kThreads;           // records per step of the accumulate scan
constexpr int kSortTile = 2048;            // records per workgroup of a radix pass (8 rounds of 256)
constexpr int kScanThreads = 1024;
typedef unsigned long long u64;

// maskApi.c bbIou on xywh doubles
__device__ __forceinline__ double bb_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh) {
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0.0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0.0) return 0.0;
  const double i = w * h;
  const double u = (dw * dh + gw * gh) - i;
  return i / u;
}

__global__ __launch_bounds__(kThreads) void det_eval_match_kernel(DetEvalMatchArgs a) {
  __shared__ u64 s_det[kMaxDet];           // class << 42 | ~order(score) << 10 | index, sorted ascending
  __shared__ u64 s_gt[kMaxGt];             // class << 10 | index, sorted ascending
  __shared__ float4 s_gbox[kMaxGt];        // by sorted position (64 KiB of LDS with the rest)
  __shared__ u64 s_match[kMaxDet], s_ignore[kMaxDet];   // by sorted position
  __shared__ int s_dstart[1024], s_dcnt[1024], s_gstart[1024], s_gcnt[1024];   // by class
  const int img = blockIdx.x, tid = threadIdx.x, C = a.n_cls;
  const int d0 = a.det_off[img], D = a.det_off[img + 1] - d0;
  const int g0 = a.gt_off[img], G = a.gt_off[img + 1] - g0;
  if (D <= 0 && G <= 0) return;
  if (D > kMaxDet || G > kMaxGt || D < 0 || G < 0) return;   // (the ABI has refused this on the host offsets)
  for (int c = tid; c < 1024; c += kThreads) { s_dstart[c] = 0; s_dcnt[c] = 0; s_gstart[c] = 0; s_gcnt[c] = 0; }
  for (int p = tid; p < D; p += kThreads) { s_match[p] = 0ull; s_ignore[p] = 0ull; }
  uint8_t* gtm = a.gtm + (size_t)g0 * kTA;
  for (int i = tid; i < G * kTA; i += kThreads) gtm[i] = 0;
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < D; i += kThreads) {
    const int64_t lab = a.det_labels[d0 + i];
    const bool ok = lab >= 1 && lab < C;
    bad += !ok;
    const u64 cls = ok ? (u64)lab : 0ull;
    s_det[i] = (cls << 42) | ((u64)(~float_order(a.det_scores[d0 + i])) << 10) | (u64)i;
    atomicAdd(&s_dcnt[(int)cls], 1);
  }
  for (int g = tid; g < G; g += kThreads) {
    const int64_t lab = a.gt_labels[g0 + g];
    const bool ok = lab >= 1 && lab < C;
    bad += !ok;
    const u64 cls = ok ? (u64)lab : 0ull;
    s_gt[g] = (cls << 10) | (u64)g;
    atomicAdd(&s_gcnt[(int)cls], 1);
    if (ok) {   // vg_eval.py:75: the annotation's area, in double
      const float* b = a.gt_boxes + 4 * (size_t)(g0 + g);
      const double area = (((double)b[3] - (double)b[1]) + 1.0) * (((double)b[2] - (double)b[0]) + 1.0);
      for (int r = 0; r < kA; ++r)
        if (!(area < a.area_rngs[2 * r] || area > a.area_rngs[2 * r + 1])) atomicAdd(&a.npig[(size_t)(lab - 1) * kA + r], 1ull);
    }
  }
  if (bad && a.label_errors) atomicAdd(a.label_errors, bad);
  __syncthreads();
  bitonic_sort(s_det, D);
  bitonic_sort(s_gt, G);
  for (int p = tid; p < D; p += kThreads) {
    const int c = (int)(s_det[p] >> 42);
    if (p == 0 || c != (int)(s_det[p - 1] >> 42)) s_dstart[c] = p;
  }
  for (int p = tid; p < G; p += kThreads) {
    const int c = (int)(s_gt[p] >> 10);
    if (p == 0 || c != (int)(s_gt[p - 1] >> 10)) s_gstart[c] = p;
  }
  __syncthreads();
  // what depends on the GT box alone, staged once by sorted position: its float32 corners and, in bits 32..35 of its key (the
  // class in the key is not read again), "ignored for area range r"
  for (int p = tid; p < G; p += kThreads) {
    const float* q = a.gt_boxes + 4 * (size_t)(g0 + (int)(s_gt[p] & 1023ull));
    const float4 b = make_float4(q[0], q[1], q[2], q[3]);
    const double g_area = (((double)b.w - (double)b.y) + 1.0) * (((double)b.z - (double)b.x) + 1.0);   // gh * gw
    u64 ig = 0ull;
    for (int r = 0; r < kA; ++r)
      if (g_area < a.area_rngs[2 * r] || g_area > a.area_rngs[2 * r + 1]) ig |= 1ull << r;
    s_gbox[p] = b;
    s_gt[p] |= ig << 32;
  }
  __syncthreads();

  // ---- COCOeval.evaluateImg: a thread per (class, threshold, area); the area index runs fastest, so a wave's lanes share a class
  for (int task = tid; task < (C - 1) * kTA; task += kThreads) {
    const int c = task / kTA + 1, ta = task % kTA, t = ta / kA, ar = ta % kA;
    const int nd = s_dcnt[c] < kCut ? s_dcnt[c] : kCut;
    if (nd == 0) continue;
    const int ng = s_gcnt[c], ds = s_dstart[c], gs = s_gstart[c];
    const double thr = fmin(a.iou_thrs[t], 1.0 - 1e-10), lo = a.area_rngs[2 * ar], hi = a.area_rngs[2 * ar + 1];
    const u64 bit = 1ull << ta;
    for (int r = 0; r < nd; ++r) {
      const int i = (int)(s_det[ds + r] & 1023ull);
      const float* b = a.det_boxes + 4 * (size_t)(d0 + i);
      const double dx = (double)b[0], dy = (double)b[1];
      const double dw = (double)((b[2] - b[0]) + 1.f), dh = (double)((b[3] - b[1]) + 1.f);   // BoxList.convert('xywh'): float32
      const double d_area = dw * dh;
      const bool d_out = d_area < lo || d_area > hi;
      int m = -1;
      bool m_ig = false;
      double best = thr;
      for (int pass = 0; pass < 2 && m < 0; ++pass)       // non-ignored GT boxes, then -- holding no match -- the ignored ones
        for (int j = 0; j < ng; ++j) {
          const u64 gk = s_gt[gs + j];
          const int g = (int)(gk & 1023ull);
          const bool g_ig = (gk >> (32 + ar)) & 1ull;
          if ((int)g_ig != pass) continue;
          const float4 q = s_gbox[gs + j];
          const double gx = (double)q.x, gy = (double)q.y;
          const double gw = ((double)q.z - gx) + 1.0, gh = ((double)q.w - gy) + 1.0;
          const double iou = bb_iou(dx, dy, dw, dh, gx, gy, gw, gh);
          if (iou < best) continue;
          if (gtm[(size_t)g * kTA + ta]) continue;   // COCOeval asks this first; the three tests commute, and this one reads global memory
          best = iou;
          m = g;
          m_ig = g_ig;
        }
      bool matched = false, ignored = d_out;
      if (m >= 0) {
        gtm[(size_t)m * kTA + ta] = 1;
        matched = a.first_gt_id + (long long)g0 + (long long)m != 0;   // COCOeval tests the stored annotation id for truth
        ignored = matched ? m_ig : (m_ig || d_out);
      }
      if (matched) atomicOr(&s_match[ds + r], bit);
      if (ignored) atomicOr(&s_ignore[ds + r], bit);
    }
  }
  __syncthreads();
  for (int p = tid; p < D; p += kThreads) {
    const u64 key = s_det[p];
    const int c = (int)(key >> 42), rank = p - s_dstart[c];
    const size_t row = (size_t)a.row_offset + (size_t)d0 + (size_t)p;
    const bool counted = c != 0 && rank < kCut;
    a.rec_key[row] = counted ? ((u64)c << 32) | ((key >> 10) & 0xffffffffull) : 0ull;
    a.rec_match[row] = counted ? s_match[p] | ((u64)rank << 40) : 0ull;
    a.rec_ignore[row] = counted ? s_ignore[p] : 0ull;
  }
}

// ---- LSD radix sort: 8 bits a pass -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void det_eval_sort_hist_kernel(const u64* keys, long long n, int shift, uint32_t* hist, int n_tile) {
  __shared__ int s_h[256];
  const int tid = threadIdx.x;
  s_h[tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
  for (int i = tid; i < kSortTile; i += kThreads)
    if (base + i < n) atomicAdd(&s_h[(int)((keys[base + i] >> shift) & 255ull)], 1);
  __syncthreads();
  hist[(size_t)tid * n_tile + blockIdx.x] = (uint32_t)s_h[tid];
}

// in-place exclusive prefix sum of hist[0..total) by one workgroup, in chunks with a carry
__global__ __launch_bounds__(kScanThreads) void det_eval_sort_scan_kernel(uint32_t* hist, long long total) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  __shared__ uint32_t s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (long long base = 0; base < total; base += kScanThreads) {
    const long long i = base + tid;
    const uint32_t v = i < total ? hist[i] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t before = s_carry;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (i < total) hist[i] = before + x - v;
    __syncthreads();
    if (tid == kScanThreads - 1) s_carry = before + x;
    __syncthreads();
  }
}

// stable scatter of one tile: the order inside a tile is (round, wave, lane) = the index order
__global__ __launch_bounds__(kThreads) void det_eval_sort_scatter_kernel(const u64* kin, const uint32_t* iin, u64* kout, uint32_t* iout,
                                                                       long long n, int shift, const uint32_t* hist, int n_tile) {
  __shared__ uint32_t s_off[256];
  __shared__ uint32_t s_wc[kThreads / 64][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  s_off[tid] = hist[(size_t)tid * n_tile + blockIdx.x];
  for (int w = 0; w < kThreads / 64; ++w) s_wc[w][tid] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * kSortTile;
  for (int round = 0; round < kSortTile / kThreads; ++round) {
    const long long i = base + round * kThreads + tid;
    const bool valid = i < n;
    const u64 key = valid ? kin[i] : 0ull;
    const int d = (int)((key >> shift) & 255ull);
    u64 peers = __ballot(valid);            // the lanes of this wave that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool one = (d >> b) & 1;
      const u64 bal = __ballot(one);
      peers &= one ? bal : ~bal;
    }
    const int lane_rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid && lane_rank == 0) s_wc[wave][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t pos = s_off[d] + (uint32_t)lane_rank;
      for (int w = 0; w < wave; ++w) pos += s_wc[w][d];
      if ((long long)pos < n) {             // (always: the offsets come from the histogram of these same keys)
        kout[pos] = key;
        iout[pos] = iin ? iin[i] : (uint32_t)i;
      }
    }
    __syncthreads();
    uint32_t tot = 0;
    for (int w = 0; w < kThreads / 64; ++w) { tot += s_wc[w][tid]; s_wc[w][tid] = 0; }
    s_off[tid] += tot;
    __syncthreads();
  }
}

// seg_start[c] = first sorted record whose class is >= c, c = 0 .. n_cls (a class above n_cls - 1 cannot come from match; it is
// clamped so that no table entry is missed or overrun)
__global__ __launch_bounds__(kThreads) void det_eval_segments_kernel(const u64* keys, long long n, int n_cls, int32_t* seg_start) {
  if (n == 0) {
    for (int c = threadIdx.x; c <= n_cls; c += kThreads) seg_start[c] = 0;
    return;
  }
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  auto cls = [&](long long j) { const int c = (int)(keys[j] >> 32); return c < n_cls ? c : n_cls; };
  const int c = cls(i), prev = i > 0 ? cls(i - 1) : -1;
  for (int cc = prev + 1; cc <= c; ++cc) seg_start[cc] = (int32_t)i;
  if (i == n - 1)
    for (int cc = c + 1; cc <= n_cls; ++cc) seg_start[cc] = (int32_t)n;
}

// ---- COCOeval.accumulate for one (class, area, maxDets): the ten thresholds in one pass over the class segment -------------
__global__ __launch_bounds__(kThreads) void det_eval_accum_kernel(DetEvalAccumArgs a, const uint32_t* sorted_idx) {
  __shared__ u64 s_max[kT][kR];            // bits of max pr over the records whose rc reaches recall threshold r and no higher one
  __shared__ double s_rec[kR];
  __shared__ u64 s_wave[kThreads / 64][kT];
  __shared__ u64 s_carry[kT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.n_cls - 1, AM = kA * 3;
  const int k = blockIdx.x / AM, am = blockIdx.x % AM, ar = am / 3, mi = am % 3;
  const int max_det = mi == 0 ? 1 : mi == 1 ? 10 : kCut;
  const u64 npig_n = a.npig[(size_t)k * kA + ar];
  if (npig_n == 0) {                       // COCOeval leaves the cell at its initial -1
    for (int e = tid; e < kT * kR; e += kThreads) a.precision[((size_t)e * K + k) * AM + am] = -1.0;
    if (tid < kT) a.recall[((size_t)tid * K + k) * AM + am] = -1.0;
    return;
  }
  const double npig = (double)npig_n;
  for (int e = tid; e < kT * kR; e += kThreads) s_max[e / kR][e % kR] = 0ull;
  for (int r = tid; r < kR; r += kThreads) s_rec[r] = a.rec_thrs[r];
  if (tid < kT) s_carry[tid] = 0ull;
  __syncthreads();
  const int beg = a.seg_start[k + 1], end = a.seg_start[k + 2];
  for (int base = beg; base < end; base += kChunk) {
    const int i = base + tid;
    bool in = false;
    u64 mw = 0, gw = 0;
    if (i < end) {
      const uint32_t idx = sorted_idx[i];
      mw = a.rec_match[idx];
      gw = a.rec_ignore[idx];
      in = (int)(mw >> 40) < max_det;
    }
    u64 v[kT];                             // tp << 32 | fp, inclusive running counts
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      const int bit = t * kA + ar;
      const bool mt = (mw >> bit) & 1ull, ig = (gw >> bit) & 1ull;
      u64 x = in && !ig ? (mt ? 1ull << 32 : 1ull) : 0ull;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
      }
      v[t] = x;
      if (lane == 63) s_wave[wave][t] = x;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      u64 before = s_carry[t];
      for (int w = 0; w < wave; ++w) before += s_wave[w][t];
      v[t] += before;
      if (in) {
        const double tp = (double)(v[t] >> 32), fp = (double)(v[t] & 0xffffffffull);
        const double rc = tp / npig;
        const double pr = tp / ((fp + tp) + 2.220446049250313e-16);   // np.spacing(1)
        int lo = 0, hi = kR;               // number of recall thresholds <= rc
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_rec[mid] <= rc) lo = mid + 1; else hi = mid;
        }
        if (lo > 0) atomicMax(&s_max[t][lo - 1], (u64)__double_as_longlong(pr));   // pr >= 0: its bits order as it does
      }
    }
    __syncthreads();
    if (tid == kThreads - 1)
      for (int t = 0; t < kT; ++t) s_carry[t] = v[t];
    __syncthreads();
  }
  if (tid < kT) {
    const int t = tid;
    double run = 0.0;
    for (int r = kR - 1; r >= 0; --r) {
      run = fmax(run, __longlong_as_double((long long)s_max[t][r]));
      a.precision[(((size_t)t * kR + r) * K + k) * AM + am] = run;
    }
    a.recall[((size_t)t * K + k) * AM + am] = (double)(s_carry[t] >> 32) / npig;
  }
}

// ---- COCOeval.summarize: workgroup s forms stats[s], workgroup 12 recall@100 at IoU 0.5 --------------------------------------
__global__ __launch_bounds__(kThreads) void det_eval_stats_kernel(DetEvalAccumArgs a) {
  __shared__ double s_sum[kThreads];
  __shared__ long long s_cnt[kThreads];
  const int s = blockIdx.x, tid = threadIdx.x, K = a.n_cls - 1, AM = kA * 3;
  // (precision?, IoU threshold or 0 = all, area, maxDets index) of summarize()'s twelve lines, then vg_eval.py:177
  const bool is_ap = s < 6;
  const double iou = s == 1 || s == 12 ? 0.5 : s == 2 ? 0.75 : 0.0;
  const int ar = (s == 3 || s == 9) ? 1 : (s == 4 || s == 10) ? 2 : (s == 5 || s == 11) ? 3 : 0;
  const int mi = s == 6 ? 0 : s == 7 ? 1 : 2;
  int t0 = 0, nt = kT;
  if (iou != 0.0) {                        // np.where(iouThr == p.iouThrs): exact equality
    nt = 0;
    for (int t = 0; t < kT; ++t)
      if (a.iou_thrs[t] == iou) { t0 = t; nt = 1; break; }
  }
  const long long per_t = is_ap ? (long long)kR * K : K, total = nt * per_t;
  double sum = 0.0;
  long long cnt = 0;
  for (long long e = tid; e < total; e += kThreads) {   // e runs over (t, r, k) / (t, k): numpy's order of s[s > -1]
    const long long t = t0 + e / per_t, rest = e % per_t;
    const double x = is_ap ? a.precision[((size_t)t * kR * K + rest) * AM + ar * 3 + mi] : a.recall[((size_t)t * K + rest) * AM + ar * 3 + mi];
    if (x > -1.0) { sum += x; ++cnt; }
  }
  s_sum[tid] = sum;
  s_cnt[tid] = cnt;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double mean = s_cnt[0] ? s_sum[0] / (double)s_cnt[0] : -1.0;
    if (s < 12) a.stats[s] = mean; else a.recall50_100[0] = mean;
  }
}

}  // namespace

int det_eval_max_gt() { return kMaxGt; }
int det_eval_max_det() { return kMaxDet; }
int det_eval_scan_chunk() { return kChunk; }
int det_eval_sort_tile() { return kSortTile; }

hipError_t launch_det_eval_match(const DetEvalMatchArgs& a, hipStream_t s) {
  VETO_LAUNCH(det_eval_match_kernel, dim3(a.n_img), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_det_eval_accumulate(const DetEvalAccumArgs& a, hipStream_t s) {
  const long long n = a.n_rec;
  const int n_tile = (int)det_eval_sort_tiles(n);
  const u64* kin = a.rec_key;
  const uint32_t* iin = nullptr;           // the first pass numbers the records itself
  u64* kout = a.key_a;
  uint32_t* iout = a.idx_a;
  hipError_t e;
  for (int pass = 0; pass < 6 && n > 0; ++pass) {
    const int shift = 8 * pass;
    VETO_LAUNCH(det_eval_sort_hist_kernel, dim3(n_tile), dim3(kThreads), 0, s, kin, n, shift, a.hist, n_tile);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    VETO_LAUNCH(det_eval_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a.hist, 256ll * n_tile);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    VETO_LAUNCH(det_eval_sort_scatter_kernel, dim3(n_tile), dim3(kThreads), 0, s, kin, iin, kout, iout, n, shift, (const uint32_t*)a.hist, n_tile);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    kin = kout; iin = iout;
    kout = kout == a.key_a ? a.key_b : a.key_a;
    iout = iout == a.idx_a ? a.idx_b : a.idx_a;
  }
  const int n_blk = n > 0 ? (int)((n + kThreads - 1) / kThreads) : 1;
  VETO_LAUNCH(det_eval_segments_kernel, dim3(n_blk), dim3(kThreads), 0, s, kin, n, a.n_cls, a.seg_start);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(det_eval_accum_kernel, dim3((a.n_cls - 1) * kA * 3), dim3(kThreads), 0, s, a, iin);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(det_eval_stats_kernel, dim3(13), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
