// Segmented greedy NMS (veto_nms) and the box head's PostProcessor around it (veto_box_postprocess), all on the device.
//
// nms_kernel -- pysgg._C.nms (csrc/cuda/nms.cu) for S segments in ONE launch, one workgroup per segment:
//   * IoU = devIoU (nms.cu:13-21), +1 pixel convention, operation for operation (fp contract off);
//   * a box is suppressed by an earlier KEPT box at IoU STRICTLY GREATER than the threshold (nms.cu:60; the reference's
//     CPU twin nms_cpu.cpp:60 uses >=, its GPU results -- what users have -- use >);
//   * boxes are visited in the total order (score desc, index asc): the reference's sort is unstable, this one is not;
//     equal means equal as floats: -0.0 and +0.0 are one score (float_order gives them one key);
//   * the kept indices come back in ASCENDING index order (nms.cu:127-130), local to the segment; a cap keeps the first
//     max_keep of that ascending list (boxlist_ops.py:29-30).
//   Structure: 64-bit keys (~score key, index) are bitonic-sorted in LDS; the order moves to 16-bit indices and the key
//   region becomes the list of kept boxes.  The sorted boxes are then resolved 64 at a time: every wave tests the 64
//   candidates (one per lane) against a quarter (a sixteenth with 1024 threads) of the kept list -- the kept box is a
//   uniform LDS read, the candidate sits in registers -- and ballots its suppressions; wave 0 ORs the ballots, builds the
//   64 x 64 suppression words of the block itself (lane i: bits j > i), walks them serially (64 uniform steps) and
//   appends the survivors to the kept list.  No n x n/64 mask is ever stored and nothing leaves the device.
//   Three instantiations by capacity (LDS per workgroup): 256 boxes (6 KiB), 1024 (18 KiB), 6144 (113 KiB, 1024 threads).
//   nms_fixed_kernel is the same for fixed-capacity segments whose live counts are known only on the device (rpn.hip).
//
// PostProcessor.forward + filter_results (box_head/inference.py:51-238) for a whole batch, four launches:
//   box_decode_kernel   one wave per proposal: softmax(class_logits), BoxCoder.decode (box_coder.py:62-95) of every
//                       class, clip_to_image(remove_empty=False) (bounding_box.py:237-247) -> workspace prob / boxes
//   class_nms_kernel    one workgroup per image x class j >= 1: candidates prob > SCORE_THRESH, the NMS above, at most
//                       POST_NMS_PER_CLS_TOPN survivors in ascending row order; every other entry of column j becomes 0,
//                       so the workspace holds the reference's dist_scores = scores * inds_all (:194-199)
//   row_max_kernel      (NMS_FILTER_DUPLICATES) one wave per row: max and first arg-max of dist_scores (:200)
//   select_kernel       one workgroup per image: the detection list (duplicates filtered: rows with a nonzero maximum in row
//                       order, :201-211; else class-major, rows ascending, :212-214), the DETECTIONS_PER_IMG cut
//                       score >= (count - cap + 1)-th smallest (:216-226) by radix select -- ties stay, as in the reference
//                       -- and the gather of orig_inds, labels, scores, boxes and boxes_per_cls[orig_inds]
#include "common.h"
#include "kernels.h"
#include "selection.h"

#pragma clang fp contract(off)   // devIoU and BoxCoder.decode follow the reference operation for operation

namespace veto {

namespace {

constexpr int kNmsMaxSeg = 6144;

// devIoU (nms.cu:13-21); a = the earlier (kept) box
__device__ __forceinline__ float dev_iou(const float4 a, const float4 b) {
  const float left = fmaxf(a.x, b.x), right = fminf(a.z, b.z);
  const float top = fmaxf(a.y, b.y), bottom = fminf(a.w, b.w);
  const float width = fmaxf((right - left) + 1.f, 0.f), height = fmaxf((bottom - top) + 1.f, 0.f);
  const float inter = width * height;
  const float sa = ((a.z - a.x) + 1.f) * ((a.w - a.y) + 1.f);
  const float sb = ((b.z - b.x) + 1.f) * ((b.w - b.y) + 1.f);
  return inter / ((sa + sb) - inter);
}

constexpr int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

template <int CAP, int NT>
struct NmsLds {
  static constexpr int kKeys = pow2_at_least(CAP);
  static constexpr int kRaw = kKeys * 8 > CAP * 16 ? kKeys * 8 : CAP * 16;
  __attribute__((aligned(16))) unsigned char raw[kRaw];   // the sort keys, then the kept boxes
  uint16_t order[kKeys];                                  // sorted position -> index inside the segment
  uint32_t keep[CAP / 32];                                // bit i: box i of the segment is kept
  float4 cand[64];
  unsigned long long ballot[NT / 64];
  int wave[NT / 64];
  int nkept, nkeys;
};

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// block-wide exclusive prefix sum for NT threads
template <int NT>
__device__ __forceinline__ int block_scan(int v, int* s_wave, int* total) {
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
  for (int w = 0; w < NT / 64; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    sum += t;
  }
  __syncthreads();
  *total = sum;
  return base + x - v;
}

__device__ __forceinline__ unsigned long long nms_key(float score, int idx) {
  return ((unsigned long long)(~float_order(score)) << 32) | (unsigned)idx;   // ascending = score desc, index asc
}

// The keys of the segment's n boxes (1 <= n <= CAP) are in L.raw and L.keep is zero, both written before the call without a
// barrier; on return (after a barrier) bit i of L.keep says whether box i survives.  box_of(i) = box i of the segment.
template <int CAP, int NT, class BoxOf>
__device__ void segment_nms(NmsLds<CAP, NT>& L, int n, float thr, BoxOf box_of) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* keys = (unsigned long long*)L.raw;
  __syncthreads();
  bitonic_sort(keys, n);
  for (int t = tid; t < n; t += NT) L.order[t] = (uint16_t)(keys[t] & 0xffffu);
  if (tid == 0) L.nkept = 0;
  __syncthreads();   // the key region is free: it becomes the kept list
  float4* kept = (float4*)L.raw;
  int nkept = 0;
  for (int base = 0; base < n; base += 64) {
    const int cnt = min(64, n - base);
    const bool live = lane < cnt;
    const int idx = live ? L.order[base + lane] : 0;
    const float4 cb = live ? box_of(idx) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (wave == 0) L.cand[lane] = cb;
    bool sup = false;
    for (int k = wave; k < nkept; k += NT / 64) sup |= dev_iou(kept[k], cb) > thr;
    const unsigned long long bal = __ballot(sup && live);
    if (lane == 0) L.ballot[wave] = bal;
    __syncthreads();
    if (wave == 0) {
      unsigned long long remv = 0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) remv |= L.ballot[w];
      unsigned long long m = 0;   // bit j > lane: this box suppresses box j of the block
      if (live && !((remv >> lane) & 1))
        for (int j = lane + 1; j < cnt; ++j)
          if (dev_iou(cb, L.cand[j]) > thr) m |= 1ull << j;
      for (int i = 0; i < cnt; ++i) {
        const unsigned long long mi = shfl64(m, i);
        if (!((remv >> i) & 1)) remv |= mi;
      }
      const unsigned long long valid = cnt == 64 ? ~0ull : ((1ull << cnt) - 1);
      const unsigned long long keepm = ~remv & valid;
      if ((keepm >> lane) & 1) {
        kept[nkept + __popcll(keepm & ((1ull << lane) - 1))] = cb;
        atomicOr(&L.keep[idx >> 5], 1u << (idx & 31));
      }
      if (lane == 0) L.nkept = nkept + __popcll(keepm);
    }
    __syncthreads();
    nkept = L.nkept;
  }
}

// rank of every kept box in ascending index order: thread t owns word t of L.keep; returns the rank of its first kept box
template <int CAP, int NT>
__device__ __forceinline__ int keep_ranks(NmsLds<CAP, NT>& L, uint32_t* word, int* total) {
  static_assert(CAP / 32 <= NT, "one thread per keep word");
  *word = threadIdx.x < CAP / 32 ? L.keep[threadIdx.x] : 0u;
  return block_scan<NT>(__popc(*word), L.wave, total);
}

template <int CAP, int NT>
__global__ __launch_bounds__(NT) void nms_kernel(NmsArgs a) {
  __shared__ NmsLds<CAP, NT> L;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int off = a.seg_off[seg], n = a.seg_off[seg + 1] - off;
  if (n <= 0 || n > CAP) {   // the ABI checked the sizes on the host; never index LDS past CAP
    if (tid == 0) a.counts[seg] = 0;
    return;
  }
  for (int t = tid; t < CAP / 32; t += NT) L.keep[t] = 0;
  unsigned long long* keys = (unsigned long long*)L.raw;
  for (int t = tid; t < n; t += NT) keys[t] = nms_key(a.scores[off + t], t);
  const float4* boxes = (const float4*)a.boxes + off;
  segment_nms<CAP, NT>(L, n, a.thr, [&](int i) { return boxes[i]; });
  uint32_t word;
  int total;
  int rank = keep_ranks<CAP, NT>(L, &word, &total);
  const int limit = a.max_keep > 0 ? min(a.max_keep, total) : total;
  while (word && rank < limit) {
    a.keep[off + rank] = tid * 32 + __ffs(word) - 1;
    word &= word - 1;
    ++rank;
  }
  if (tid == 0) a.counts[seg] = limit;
}

// The same for fixed-capacity segments whose live counts exist only on the device (the RPN's candidates behind its small-box
// filter): rows s * capacity .. + live[s].
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void nms_fixed_kernel(NmsFixedArgs a) {
  __shared__ NmsLds<CAP, NT> L;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const size_t off = (size_t)seg * a.capacity;
  const int n = min(a.live[seg], min(a.capacity, CAP));   // never index LDS past CAP
  if (n <= 0) {
    if (tid == 0) a.counts[seg] = 0;
    return;
  }
  for (int t = tid; t < CAP / 32; t += NT) L.keep[t] = 0;
  unsigned long long* keys = (unsigned long long*)L.raw;
  for (int t = tid; t < n; t += NT) keys[t] = nms_key(a.scores[off + t], t);
  const float4* boxes = (const float4*)a.boxes + off;
  segment_nms<CAP, NT>(L, n, a.thr, [&](int i) { return boxes[i]; });
  uint32_t word;
  int total;
  int rank = keep_ranks<CAP, NT>(L, &word, &total);
  const int limit = a.max_keep > 0 ? min(a.max_keep, total) : total;
  while (word && rank < limit) {
    a.keep[off + rank] = tid * 32 + __ffs(word) - 1;
    word &= word - 1;
    ++rank;
  }
  if (tid == 0) a.counts[seg] = limit;
}

// ---- the box head's PostProcessor ------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void box_decode_kernel(BoxPostArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), C = a.n_cls;
  if (row >= a.n_box) return;
  int img = 0;
  while (img + 1 < a.n_img && row >= a.img_off[img + 1]) ++img;
  const float xmax = a.image_sizes[2 * img] - 1.f, ymax = a.image_sizes[2 * img + 1] - 1.f;
  // F.softmax(class_logits, -1)
  const float* logit = a.logits + (size_t)row * C;
  float mx = -INFINITY;
  for (int c = lane; c < C; c += 64) mx = fmaxf(mx, logit[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum += expf(logit[c] - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  float* prob = a.prob + (size_t)row * C;
  for (int c = lane; c < C; c += 64) prob[c] = c == 0 ? 0.f : expf(logit[c] - mx) * inv;   // column 0: inds_all[:, 0] = 0
  // BoxCoder.decode (box_coder.py:62-95), TO_REMOVE = 1
  const float4 p = ((const float4*)a.proposals)[row];
  const float w = (p.z - p.x) + 1.f, h = (p.w - p.y) + 1.f;
  const float cx = p.x + 0.5f * w, cy = p.y + 0.5f * h;
  const float* reg = a.regression + (size_t)row * a.reg_cols;
  float4* out = (float4*)a.dec + (size_t)row * C;
  for (int c = lane; c < C; c += 64) {
    const float4 r = *(const float4*)(reg + (a.cls_agnostic ? a.reg_cols - 4 : 4 * c));
    const float dx = r.x / a.wx, dy = r.y / a.wy;
    const float dw = fminf(r.z / a.ww, a.xform_clip), dh = fminf(r.w / a.wh, a.xform_clip);
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    float4 b;
    b.x = pcx - 0.5f * pw;
    b.y = pcy - 0.5f * ph;
    b.z = (pcx + 0.5f * pw) - 1.f;
    b.w = (pcy + 0.5f * ph) - 1.f;
    // clip_to_image(remove_empty=False): clamp_(min=0, max=size - 1)
    b.x = fminf(fmaxf(b.x, 0.f), xmax);
    b.y = fminf(fmaxf(b.y, 0.f), ymax);
    b.z = fminf(fmaxf(b.z, 0.f), xmax);
    b.w = fminf(fmaxf(b.w, 0.f), ymax);
    out[c] = b;
  }
}

template <int CAP, int NT>
__global__ __launch_bounds__(NT) void class_nms_kernel(BoxPostArgs a) {
  __shared__ NmsLds<CAP, NT> L;
  const int j = blockIdx.x + 1, img = blockIdx.y, tid = threadIdx.x, C = a.n_cls;
  const int off = a.img_off[img], n = a.img_off[img + 1] - off;
  if (n <= 0 || n > CAP) return;
  for (int t = tid; t < CAP / 32; t += NT) L.keep[t] = 0;
  if (tid == 0) L.nkeys = 0;
  __syncthreads();
  unsigned long long* keys = (unsigned long long*)L.raw;
  float* col = a.prob + (size_t)off * C + j;
  for (int r = tid; r < n; r += NT) {
    const float s = col[(size_t)r * C];
    if (s > a.score_thresh) keys[atomicAdd(&L.nkeys, 1)] = nms_key(s, r);   // any order: the sort's order is total
  }
  __syncthreads();
  const int m = L.nkeys;
  if (m == 0) return;   // nothing above the threshold: no entry of the column counts as a survivor
  const float4* boxes = (const float4*)a.dec + (size_t)off * C + j;
  segment_nms<CAP, NT>(L, m, a.nms_thresh, [&](int r) { return boxes[(size_t)r * C]; });
  uint32_t word;
  int total;
  int rank = keep_ranks<CAP, NT>(L, &word, &total);
  const int limit = a.topn > 0 ? min(a.topn, total) : total;
  if (tid < CAP / 32) {
    for (int b = 0; b < 32; ++b) {
      const int r = tid * 32 + b;
      if (r >= n) break;
      const bool kept = (word >> b) & 1;   // (only candidates can be kept)
      if (!(kept && rank < limit) && col[(size_t)r * C] > a.score_thresh) col[(size_t)r * C] = 0.f;
      rank += kept;
    }
  }
}

// After class_nms_kernel an entry of the probability matrix is a survivor exactly when it is > SCORE_THRESH (>= 0): suppressed
// candidates were zeroed, everything else never passed the threshold.
__global__ __launch_bounds__(256) void row_max_kernel(BoxPostArgs a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), C = a.n_cls;
  if (row >= a.n_box) return;
  const float* prob = a.prob + (size_t)row * C;
  float best = 0.f;            // dist_scores.max(1): column 0 is 0, first column on ties
  int col = 0;
  for (int c = lane; c < C; c += 64) {
    const float v = prob[c] > a.score_thresh ? prob[c] : 0.f;
    if (v > best) { best = v; col = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(col, o, 64);
    if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
  }
  if (lane == 0) { a.row_score[row] = best; a.row_label[row] = col; }
}

__global__ __launch_bounds__(256) void select_kernel(BoxPostArgs a) {
  __shared__ SelLds sel;
  const int img = blockIdx.x, tid = threadIdx.x, C = a.n_cls;
  const int off = a.img_off[img], n = a.img_off[img + 1] - off;
  const int out0 = a.out_off[img], capacity = a.out_off[img + 1] - out0;
  const size_t list0 = a.filter_dup ? (size_t)off : (size_t)off * (C - 1);
  float* l_score = a.list_score + list0;
  int32_t* l_row = a.list_row + list0;
  int32_t* l_label = a.list_label + list0;
  int total = 0;
  if (a.filter_dup) {   // rows with a nonzero maximum, ascending (inference.py:200-211)
    for (int base = 0; base < n; base += 256) {
      const int r = base + tid;
      const float s = r < n ? a.row_score[off + r] : 0.f;
      const int flag = s != 0.f;
      int cnt;
      const int pos = total + block_exclusive_scan(flag, sel.wave, &cnt);
      if (flag) { l_score[pos] = s; l_row[pos] = r; l_label[pos] = a.row_label[off + r]; }
      total += cnt;
    }
  } else {              // class-major, rows ascending (:212-214): thread c owns column c
    for (int cbase = 1; cbase < C; cbase += 256) {
      const int c = cbase + tid;
      const float* col = a.prob + (size_t)off * C + c;
      int mine = 0;
      if (c < C)
        for (int r = 0; r < n; ++r) mine += col[(size_t)r * C] > a.score_thresh;
      int cnt;
      int pos = total + block_exclusive_scan(mine, sel.wave, &cnt);
      if (c < C)
        for (int r = 0; r < n; ++r) {
          const float s = col[(size_t)r * C];
          if (s > a.score_thresh) { l_score[pos] = s; l_row[pos] = r; l_label[pos] = c; ++pos; }
        }
      total += cnt;
    }
  }
  __syncthreads();   // the lists (global memory, this workgroup's own) are read back below
  // the cut: keep score >= the (total - cap + 1)-th smallest = the cap-th largest (:216-226); ties at that value stay
  const int per = (total + 255) / 256;
  const int lo = min(total, tid * per), hi = min(total, lo + per);
  uint32_t T = 0;
  if (a.det_per_img > 0 && total > a.det_per_img) {
    int need;
    radix_select([&](auto f) { for (int i = lo; i < hi; ++i) f(float_order(l_score[i])); }, a.det_per_img, sel, T, need);
  }
  int mine = 0;
  for (int i = lo; i < hi; ++i) mine += float_order(l_score[i]) >= T;
  int fc;
  int pos = block_exclusive_scan(mine, sel.wave, &fc);
  if (fc > capacity) {   // the caller's rows do not hold the result: report the count, write nothing
    if (tid == 0) a.counts[img] = -fc;
    return;
  }
  for (int i = lo; i < hi; ++i) {
    if (float_order(l_score[i]) < T) continue;
    const int r = l_row[i], lab = l_label[i];
    a.orig_inds[out0 + pos] = r;
    a.labels[out0 + pos] = lab;
    a.scores[out0 + pos] = l_score[i];
    ((float4*)a.boxes)[out0 + pos] = ((const float4*)a.dec)[(size_t)(off + r) * C + lab];
    ++pos;
  }
  if (tid == 0) a.counts[img] = fc;
  if (!a.boxes_per_cls) return;
  __syncthreads();   // orig_inds of this image are visible to the whole workgroup
  for (int t = tid; t < fc * C; t += 256) {
    const int d = t / C, c = t - d * C;
    ((float4*)a.boxes_per_cls)[(size_t)(out0 + d) * C + c] = ((const float4*)a.dec)[(size_t)(off + (int)a.orig_inds[out0 + d]) * C + c];
  }
}

}  // namespace

int nms_max_segment() { return kNmsMaxSeg; }

hipError_t launch_nms(const NmsArgs& a, int max_seg, hipStream_t s) {
  if (max_seg <= 256) VETO_LAUNCH((nms_kernel<256, 256>), dim3(a.n_seg), dim3(256), 0, s, a);
  else if (max_seg <= 1024) VETO_LAUNCH((nms_kernel<1024, 256>), dim3(a.n_seg), dim3(256), 0, s, a);
  else VETO_LAUNCH((nms_kernel<kNmsMaxSeg, 1024>), dim3(a.n_seg), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_nms_fixed(const NmsFixedArgs& a, hipStream_t s) {
  if (a.capacity <= 256) VETO_LAUNCH((nms_fixed_kernel<256, 256>), dim3(a.n_seg), dim3(256), 0, s, a);
  else if (a.capacity <= 1024) VETO_LAUNCH((nms_fixed_kernel<1024, 256>), dim3(a.n_seg), dim3(256), 0, s, a);
  else VETO_LAUNCH((nms_fixed_kernel<kNmsMaxSeg, 1024>), dim3(a.n_seg), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_box_postprocess(const BoxPostArgs& a, int max_per_img, hipStream_t s) {
  VETO_LAUNCH(box_decode_kernel, dim3((a.n_box + 3) / 4), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid(a.n_cls - 1, a.n_img);
  if (max_per_img <= 256) VETO_LAUNCH((class_nms_kernel<256, 256>), grid, dim3(256), 0, s, a);
  else if (max_per_img <= 1024) VETO_LAUNCH((class_nms_kernel<1024, 256>), grid, dim3(256), 0, s, a);
  else VETO_LAUNCH((class_nms_kernel<kNmsMaxSeg, 1024>), grid, dim3(1024), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.filter_dup) {
    VETO_LAUNCH(row_max_kernel, dim3((a.n_box + 3) / 4), dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  VETO_LAUNCH(select_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
