// Detector training, the RPN loss: RPNLossComputation (pysgg/modeling/rpn/loss.py:21-157) for a ragged batch.  The reference loops
// over the images on the host: a [n_gt, n_anchor] boxlist_iou matrix, max over both axes, a nonzero over an equality mask of the
// whole matrix, two nonzero / randperm pairs, and after the loop a permute + concatenate of every level's NCHW outputs to gather
// 256 rows per image.  Here the matrix is never stored, the head outputs are read and their gradients written in place in NCHW,
// and the loss normaliser (the count of sampled anchors) stays on the device.  Seven launches whatever the batch or the pyramid:
//
//   rpn_loss_fill_kernel     zeroes the per-GT maxima, the sampler's histograms and, when gradients are asked for, every level's
//                            gradient tensor.
//   rpn_match_kernel<1>      grid (tile of 256 anchors, image).  The image's GT boxes (<= 256) are staged in LDS; one thread owns one
//                            anchor and walks them in index order with selection.h::boxlist_iou.  highest_quality_foreach_gt
//                            (matcher.py:92): an integer atomicMax on the IoU's bit pattern in LDS, then one per GT and workgroup in
//                            memory.  IoU is never negative, so the unsigned pattern orders like the value, and an integer maximum
//                            does not depend on arrival order.
//   rpn_match_kernel<2>      the same walk again (cheaper than keeping 8 bytes per anchor between the passes): the maximum and,
//                            with a strict `>`, the lowest GT index reaching it (max(dim=0) on the CPU); Matcher's thresholds
//                            (matcher.py:71-76); set_low_quality_matches_ (:83-112): an anchor whose IoU with any GT j equals gtmax[j]
//                            -- recomputed by the same function, so the equality is exact -- gets its argmax back, which for a GT that
//                            overlaps nothing (gtmax 0) is every anchor with IoU 0 to it, as in the reference; the labels in the order
//                            of loss.py:65-79 with the visibility of anchor_generator.py:97-110; BoxCoder.encode when asked for.
//   rpn_hist_kernel          grid (tile of 8192 anchors, image): BalancedPositiveNegativeSampler with the convention of
//                            box_subsample_kernel -- a class above its quota keeps the `quota` smallest (hash, anchor index), hash =
//                            upper 32 bits of rng64(seed, image, class, anchor) -- starts as a histogram of the keys' top 8 bits per
//                            image and class, integer adds only.
//   rpn_sample_kernel        one workgroup per image.  The histogram gives the class sizes, the quotas and the cut bin.  Then one
//                            coalesced pass over the labels: anchors above the cut bin are taken, those inside it (<= 2048, some
//                            0.4 % of the class) are sorted in LDS by (hash, anchor index) and the best fill the quota; the taken
//                            anchors (<= 2048) are sorted and leave in ascending order.  A cut bin that does not fit (above
//                            about half a million anchors of one class) takes the streaming path instead: the radix select of
//                            selection.h over the labels in memory, then one block scan per 256 consecutive anchors.
//   rpn_loss_kernel          one workgroup per image over its sampled anchors (ascending, so neighbouring lanes read neighbouring
//                            cells of the NCHW tensors where the sample allows): BCE-with-logits and smooth-L1 terms and their
//                            gradients / S, in double from the fp32 inputs; fixed-order sums into one partial pair per image.
//   rpn_loss_final_kernel    sums the partials in image order and divides by S.  No floating-point atomics anywhere.
#include "common.h"
#include "kernels.h"
#include "selection.h"

namespace veto {

namespace {

constexpr int kMaxGt = 256;            // GT boxes per image: the LDS stage
constexpr int kMaxAnchors = 1 << 20;   // anchors per image
constexpr int kMaxBatch = 2048;        // BATCH_SIZE_PER_IMAGE
constexpr int kTile = 256;
constexpr int kFillBlocks = 512;       // workgroups per zero-filled tensor
constexpr int kHistTile = 8192;        // anchors per workgroup of the sampler's histogram
constexpr int kCandCap = 2048;         // keys of one cut bin the sampler sorts in LDS

enum { kPickPos = 0, kPickNeg = 1 };   // the class codes of box_subsample_kernel

// the descriptor table into LDS, with constant indices into the kernel arguments; the caller synchronises
__device__ __forceinline__ void stage_levels(const RpnLossArgs& a, RpnLossLevel* s_lvl) {
#pragma unroll
  for (int l = 0; l < kRpnMaxLevels; ++l)
    if ((int)threadIdx.x == l) s_lvl[l] = a.lvl[l];
}

// the level that holds image-anchor i (the levels are few: a walk over their first indices)
__device__ __forceinline__ int level_of(const RpnLossLevel* s_lvl, int n_lvl, int i) {
  int l = 0;
  while (l + 1 < n_lvl && i >= s_lvl[l + 1].off) ++l;
  return l;
}

__device__ __forceinline__ float4 anchor_box(const RpnLossLevel& lv, int i) {
  return reinterpret_cast<const float4*>(lv.anchors)[i - lv.off];
}

__global__ __launch_bounds__(256) void rpn_loss_fill_kernel(RpnFillArgs a) {
  float* p = a.ptr[blockIdx.y];
  const long long n = a.n[blockIdx.y], groups = (n + 3) / 4;
  const bool vec = ((uintptr_t)p & 15) == 0;
  for (long long g = blockIdx.x * 256ll + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
    const long long e = g * 4;
    if (vec && e + 4 <= n) {
      reinterpret_cast<float4*>(p)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (long long k = e; k < n && k < e + 4; ++k) p[k] = 0.f;
    }
  }
}

template <int PASS>
__global__ __launch_bounds__(kTile) void rpn_match_kernel(RpnLossArgs a) {
  __shared__ float4 s_gt[kMaxGt];
  __shared__ uint32_t s_max[kMaxGt];   // pass 1: this workgroup's maxima; pass 2: gtmax
  __shared__ RpnLossLevel s_lvl[kRpnMaxLevels];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int t0 = a.tgt_off[img], m = a.tgt_off[img + 1] - t0;
  if (m <= 0 || m > kMaxGt) return;   // the ABI checks the host-side sizes; never index LDS past 256 rows
  stage_levels(a, s_lvl);
  const float4* gt = reinterpret_cast<const float4*>(a.tgt_boxes) + t0;
  for (int j = tid; j < m; j += kTile) {
    s_gt[j] = gt[j];
    s_max[j] = PASS == 1 ? 0u : a.gtmax[t0 + j];
  }
  __syncthreads();
  const int i = blockIdx.x * kTile + tid;
  const bool live = i < a.n_anchor;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) p = anchor_box(s_lvl[level_of(s_lvl, a.n_lvl, i)], i);
  const float pb[4] = {p.x, p.y, p.z, p.w};

  if (PASS == 1) {
    if (live) {
      volatile uint32_t* seen = s_max;
      for (int j = 0; j < m; ++j) {
        const float4 g = s_gt[j];
        const float gb[4] = {g.x, g.y, g.z, g.w};
        const uint32_t bits = __float_as_uint(boxlist_iou(gb, pb));
        if (bits > seen[j]) atomicMax(&s_max[j], bits);   // most pairs do not overlap: the read filters them
      }
    }
    __syncthreads();
    for (int j = tid; j < m; j += kTile)
      if (s_max[j]) atomicMax(&a.gtmax[t0 + j], s_max[j]);
    return;
  }

  if (!live) return;
  float best = 0.f;
  int arg = 0;
  bool lowq = false;
  for (int j = 0; j < m; ++j) {
    const float4 g = s_gt[j];
    const float gb[4] = {g.x, g.y, g.z, g.w};
    const float iou = boxlist_iou(gb, pb);
    if (j == 0 || iou > best) { best = iou; arg = j; }
    lowq |= iou == __uint_as_float(s_max[j]);             // match_quality_matrix == highest_quality_foreach_gt[:, None]
  }
  int matched = arg;
  if (best < a.low) matched = -1;                          // Matcher.BELOW_LOW_THRESHOLD
  else if (best < a.high) matched = -2;                    // Matcher.BETWEEN_THRESHOLDS
  if (a.allow_lowq && lowq) matched = arg;                 // matches[pred_inds_to_update] = all_matches[...]
  const float iw = a.image_sizes[2 * img], ih = a.image_sizes[2 * img + 1];
  const bool visible = a.straddle < 0.f || (p.x >= -a.straddle && p.y >= -a.straddle && p.z < iw + a.straddle && p.w < ih + a.straddle);
  // loss.py:65-79: 1 where matched >= 0, 0 where -1, then -1 where not visible, then -1 where -2
  const float label = (!visible || matched == -2) ? -1.f : (matched >= 0 ? 1.f : 0.f);
  const size_t row = (size_t)img * a.n_anchor + i;
  a.labels_ws[row] = label;
  a.matched_ws[row] = matched;
  if (a.matched) a.matched[row] = matched;
  if (a.targets) reinterpret_cast<float4*>(a.targets)[row] = encode_box(s_gt[matched < 0 ? 0 : matched], p, a.wx, a.wy, a.ww, a.wh);
}

// the sampler's class and key of anchor e: class -1 is ignored
__device__ __forceinline__ int label_class(float l) { return l >= 1.f ? 0 : (l == 0.f ? 1 : -1); }
__device__ __forceinline__ uint32_t sample_key(const RpnLossArgs& a, int img, int c, int e) {
  return ~(uint32_t)(rng64(a.seed, img, c == 0 ? kPickPos : kPickNeg, (uint32_t)e) >> 32);
}

// per image and class the histogram of the keys' top 8 bits: LDS first, then one integer add per non-empty bin and workgroup
__global__ __launch_bounds__(256) void rpn_hist_kernel(RpnLossArgs a) {
  __shared__ int s_hist[2][256];
  const int img = blockIdx.y, tid = threadIdx.x, n = a.n_anchor;
  const float* lab = a.labels_ws + (size_t)img * n;
  s_hist[0][tid] = 0;
  s_hist[1][tid] = 0;
  __syncthreads();
  const int e1 = min(n, ((int)blockIdx.x + 1) * kHistTile);
  for (int e = blockIdx.x * kHistTile + tid; e < e1; e += 256) {
    const int c = label_class(lab[e]);
    if (c >= 0) atomicAdd(&s_hist[c][sample_key(a, img, c, e) >> 24], 1);
  }
  __syncthreads();
  for (int c = 0; c < 2; ++c)
    if (s_hist[c][tid]) atomicAdd(&a.hist[((size_t)img * 2 + c) * 256 + tid], s_hist[c][tid]);
}

__global__ __launch_bounds__(256) void rpn_sample_kernel(RpnLossArgs a) {
  __shared__ SelLds s_sel;
  __shared__ unsigned long long s_cand[2][kCandCap];   // per class the keys of its cut bin
  __shared__ unsigned long long s_take[kMaxBatch];  // the anchors taken
  __shared__ int s_count[3];                           // entries of s_cand[0], s_cand[1], s_take
  const int img = blockIdx.x, tid = threadIdx.x, n = a.n_anchor;
  const float* lab = a.labels_ws + (size_t)img * n;
  const int* hist = a.hist + (size_t)img * 512;
  int m_pos, m_neg;
  (void)block_exclusive_scan(hist[tid], s_sel.wave, &m_pos);
  (void)block_exclusive_scan(hist[256 + tid], s_sel.wave, &m_neg);
  const int num_pos = min(m_pos, a.num_pos);               // balanced_positive_negative_sampler.py:41-46
  const int num_neg = min(m_neg, a.batch - num_pos);
  int32_t* out = a.sampled_ws + (size_t)img * a.batch;
  int64_t* out64 = a.sampled ? a.sampled + (size_t)img * a.batch : nullptr;
  if (tid == 0) {
    a.counts_ws[2 * img] = num_pos;
    a.counts_ws[2 * img + 1] = num_neg;
    if (a.counts) {
      a.counts[2 * img] = num_pos;
      a.counts[2 * img + 1] = num_neg;
    }
  }

  // per class: 0 none of it, 1 all of it, 2 a draw: the keys above the cut bin (top 8 bits) and the `bin_need` best of that bin
  int mode[2], cut[2] = {0, 0}, bin_need[2] = {0, 0};
  const int quota[2] = {num_pos, num_neg}, members[2] = {m_pos, m_neg};
  bool small_bins = true;
  for (int c = 0; c < 2; ++c) {
    mode[c] = quota[c] <= 0 ? 0 : (quota[c] >= members[c] ? 1 : 2);
    if (mode[c] != 2) continue;
    const int h = hist[c * 256 + 255 - tid];   // an ascending scan over descending digits
    int dummy;
    const int above = block_exclusive_scan(h, s_sel.wave, &dummy);
    if (above < quota[c] && above + h >= quota[c]) { s_sel.digit = 255 - tid; s_sel.need = quota[c] - above; }
    __syncthreads();
    cut[c] = s_sel.digit;
    bin_need[c] = s_sel.need;
    small_bins &= hist[c * 256 + cut[c]] <= kCandCap;
    __syncthreads();
  }

  if (small_bins) {
    // One coalesced pass, no barrier inside: an anchor above its class's cut bin is taken, one inside it is a candidate.  Both
    // lists fill in arrival order and are sorted afterwards, so the rows do not depend on it.  Candidates sort by (key
    // descending, anchor ascending): the first bin_need of them are the members with the smallest (hash, anchor index).
    if (tid < 3) s_count[tid] = 0;
    __syncthreads();
    constexpr int kAhead = 8;   // labels in flight per thread: the pass is bound by their latency
    for (int base = 0; base < n; base += kAhead * 256) {
      float l[kAhead];
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        const int e = base + k * 256 + tid;
        l[k] = e < n ? lab[e] : -1.f;
      }
#pragma unroll
      for (int k = 0; k < kAhead; ++k) {
        const int e = base + k * 256 + tid, c = label_class(l[k]);
        if (c < 0 || mode[c] == 0) continue;
        bool take = mode[c] == 1;
        if (!take) {
          const uint32_t key = sample_key(a, img, c, e);
          const int digit = key >> 24;
          take = digit > cut[c];
          if (digit == cut[c]) {
            const int slot = atomicAdd(&s_count[c], 1);
            if (slot < kCandCap) s_cand[c][slot] = ((unsigned long long)(~key) << 32) | (uint32_t)e;
          }
        }
        if (take) {
          const int slot = atomicAdd(&s_count[2], 1);
          if (slot < kMaxBatch) s_take[slot] = (uint32_t)e;
        }
      }
    }
    __syncthreads();
    for (int c = 0; c < 2; ++c) {
      if (mode[c] != 2) continue;
      bitonic_sort(s_cand[c], min(s_count[c], kCandCap));
      const int base = s_count[2];
      __syncthreads();
      for (int t = tid; t < bin_need[c]; t += 256)
        if (base + t < kMaxBatch) s_take[base + t] = s_cand[c][t] & 0xffffffffull;
      if (tid == 0) s_count[2] = base + bin_need[c];
      __syncthreads();
    }
    __syncthreads();
    const int total = min(s_count[2], a.batch);
    bitonic_sort(s_take, total);
    for (int t = tid; t < total; t += 256) {
      out[t] = (int32_t)s_take[t];
      if (out64) out64[t] = (int64_t)s_take[t];
    }
    return;
  }

  // A cut bin too large for LDS (about half a million anchors of one class and more): the full radix select, then the survivors
  // through one block scan per 256 consecutive anchors.
  uint32_t T[2] = {0, 0};
  int need[2] = {0, 0};
  for (int c = 0; c < 2; ++c) {
    if (mode[c] != 2) continue;
    auto keys = [&](auto f) {   // strided: a histogram does not depend on the order of its elements
      for (int e = tid; e < n; e += 256)
        if (label_class(lab[e]) == c) f(sample_key(a, img, c, e));
    };
    radix_select(keys, quota[c], s_sel, T[c], need[c]);
  }

  // the survivors in ascending anchor order: one scan per 256 consecutive anchors carries three counts, the anchors taken
  // outright (bits 0-9), the positives with key == T (10-19) and the negatives with key == T (20-29)
  int out_run = 0, eq_run[2] = {0, 0};
  constexpr int kAhead = 4;   // tiles whose labels are loaded before the first of their scans
  for (int base = 0; base < n; base += kAhead * 256) {
    float l[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      const int e = base + k * 256 + tid;
      l[k] = e < n ? lab[e] : -1.f;
    }
#pragma unroll
    for (int k = 0; k < kAhead; ++k) {
      if (base + k * 256 >= n) break;
      const int e = base + k * 256 + tid;
      const int c = label_class(l[k]);
      int sure = 0, eq = 0;
      if (c >= 0) {
        if (mode[c] == 1) {
          sure = 1;
        } else if (mode[c] == 2) {
          const uint32_t key = sample_key(a, img, c, e);
          sure = key > T[c];
          eq = key == T[c];
        }
      }
      int total;
      const int before = block_exclusive_scan(sure | (eq << (c == 0 ? 10 : 20)), s_sel.wave, &total);
      const int room[2] = {max(need[0] - eq_run[0], 0), max(need[1] - eq_run[1], 0)};
      const int eq_before[2] = {(before >> 10) & 1023, (before >> 20) & 1023};
      const int eq_total[2] = {(total >> 10) & 1023, (total >> 20) & 1023};
      const bool take = sure || (eq && eq_before[c == 0 ? 0 : 1] < room[c == 0 ? 0 : 1]);
      const int slot = out_run + (before & 1023) + min(eq_before[0], room[0]) + min(eq_before[1], room[1]);
      if (take && slot < a.batch) {
        out[slot] = e;
        if (out64) out64[slot] = e;
      }
      out_run += (total & 1023) + min(eq_total[0], room[0]) + min(eq_total[1], room[1]);
      eq_run[0] += eq_total[0];
      eq_run[1] += eq_total[1];
    }
  }
}

// S = the sampled anchors of the whole batch: an integer sum, the same in every workgroup
__device__ __forceinline__ int batch_sampled(const RpnLossArgs& a, int* s_wave) {
  int mine = 0;
  for (int i = threadIdx.x; i < a.n_img; i += 256) mine += a.counts_ws[2 * i] + a.counts_ws[2 * i + 1];
  int S;
  (void)block_exclusive_scan(mine, s_wave, &S);
  return S;
}

// both sums of the workgroup in a fixed order: thread 0 returns them
__device__ __forceinline__ void block_sum2(double& x, double& y, double (*s_red)[256]) {
  s_red[0][threadIdx.x] = x;
  s_red[1][threadIdx.x] = y;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s_red[0][threadIdx.x] += s_red[0][threadIdx.x + w];
      s_red[1][threadIdx.x] += s_red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  x = s_red[0][0];
  y = s_red[1][0];
}

__global__ __launch_bounds__(256) void rpn_loss_kernel(RpnLossArgs a) {
  __shared__ double s_red[2][256];
  __shared__ int s_wave[4];
  __shared__ RpnLossLevel s_lvl[kRpnMaxLevels];
  const int img = blockIdx.x, tid = threadIdx.x;
  stage_levels(a, s_lvl);
  const int S = batch_sampled(a, s_wave);   // (its barriers publish s_lvl)
  const int cnt = min(a.counts_ws[2 * img] + a.counts_ws[2 * img + 1], a.batch);
  const double inv = 1.0 / (double)S, beta = a.beta;
  const int t0 = a.tgt_off[img];
  double obj = 0.0, box = 0.0;
  for (int k = tid; k < cnt; k += 256) {
    const int i = a.sampled_ws[(size_t)img * a.batch + k];
    if (i < 0 || i >= a.n_anchor) continue;   // never index the head outputs past their ends
    const RpnLossLevel& lv = s_lvl[level_of(s_lvl, a.n_lvl, i)];
    const int local = i - lv.off, cell = local / lv.A, an = local - cell * lv.A;   // anchor (h W + w) A + a
    const size_t row = (size_t)img * a.n_anchor + i;
    const bool pos = a.labels_ws[row] >= 1.f;
    const size_t o = ((size_t)img * lv.A + an) * lv.HW + cell;                      // objectness[img, a, h, w]
    const double x = lv.objectness[o];
    obj += fmax(x, 0.0) - (pos ? x : 0.0) + log1p(exp(-fabs(x)));
    if (lv.d_objectness) lv.d_objectness[o] = (float)((pos ? -1.0 / (1.0 + exp(x)) : 1.0 / (1.0 + exp(-x))) * inv);   // sigmoid(x) - y
    if (!pos) continue;
    const int g = max(a.matched_ws[row], 0);
    const float4 t = encode_box(reinterpret_cast<const float4*>(a.tgt_boxes)[t0 + g], anchor_box(lv, i), a.wx, a.wy, a.ww, a.wh);
    const float tc[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const size_t r = ((size_t)img * 4 * lv.A + 4 * an + c) * lv.HW + cell;        // box_regression[img, 4 a + c, h, w]
      const double d = (double)lv.regression[r] - (double)tc[c], ad = fabs(d);
      box += ad < beta ? 0.5 * d * d / beta : ad - 0.5 * beta;
      if (lv.d_regression) lv.d_regression[r] = (float)((ad < beta ? d / beta : (d > 0.0 ? 1.0 : -1.0)) * inv);
    }
  }
  block_sum2(obj, box, s_red);
  if (tid == 0) {
    a.partial[2 * img] = obj;
    a.partial[2 * img + 1] = box;
  }
}

__global__ __launch_bounds__(256) void rpn_loss_final_kernel(RpnLossArgs a) {
  __shared__ double s_red[2][256];
  __shared__ int s_wave[4];
  const int S = batch_sampled(a, s_wave);
  double obj = 0.0, box = 0.0;
  for (int i = threadIdx.x; i < a.n_img; i += 256) {
    obj += a.partial[2 * i];
    box += a.partial[2 * i + 1];
  }
  block_sum2(obj, box, s_red);
  if (threadIdx.x == 0 && a.losses) {   // S = 0: the mean of nothing, NaN, as the reference's
    a.losses[0] = (float)(obj / (double)S);
    a.losses[1] = (float)(box / (double)S);
  }
}

}  // namespace

int rpn_loss_max_gt() { return kMaxGt; }
int rpn_loss_max_anchors() { return kMaxAnchors; }
int rpn_loss_max_batch() { return kMaxBatch; }

hipError_t launch_rpn_loss(const RpnLossArgs& a, const RpnFillArgs& fill, int last_stage, hipStream_t s) {
  const dim3 tiles((a.n_anchor + kTile - 1) / kTile, a.n_img);
  hipError_t e;
  VETO_LAUNCH(rpn_loss_fill_kernel, dim3(kFillBlocks, fill.n_seg), dim3(256), 0, s, fill);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(rpn_match_kernel<1>, tiles, dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(rpn_match_kernel<2>, tiles, dim3(kTile), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess || last_stage < kRpnLossSample) return e;
  VETO_LAUNCH(rpn_hist_kernel, dim3((a.n_anchor + kHistTile - 1) / kHistTile, a.n_img), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(rpn_sample_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess || last_stage < kRpnLossLoss) return e;
  VETO_LAUNCH(rpn_loss_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(rpn_loss_final_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
