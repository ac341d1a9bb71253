// SGDet (detected boxes) around the relation predictor: the two host loops of the reference that need
// the detector's boxes, as one workgroup per image each.
//
// obj_decode_kernel -- greedy class-aware NMS over the [N, C] class probabilities:
//   mode 0: obj_prediction_nms (pysgg/modeling/roi_heads/relation_head/utils_relation.py:94-128), the
//           PostProcessor's object decoding (inference.py:410-429; also :123-147 and :317-341)
//   mode 1: Ensemble.nms_per_cls (roi_relation_predictors.py:3855-3874), the MEET decoder's label lookup, on
//           softmax(one_hot(labels)): only the order hot > cold > 0 > -1 and the exact ties between rows matter, so
//           every row is built from the same two values (1 and 1/2) -- ties go to the first row-major index
//   prob = softmax(logits); prob[:, 0] = 0 (mode 0) or -1 (mode 1); repeat N times:
//     (b, c) = first row-major arg-max of prob (numpy argmax)
//     label[b] = c            (mode 0: only while label[b] == 0)
//     prob[j, c] = 0 for every j with IoU(box[b, c], box[j, c]) >= thr  (nms_overlaps, :56-92)
//     prob[b, :] = -1
//   The N x N x C overlap tensor of the reference is never built: a step computes the N IoUs of column c
//   against box b.  Row maxima (value, first column) live in LDS; a step picks (value desc, row asc) with
//   one wave and updates only the rows whose entry in column c changed (a full rescan only when that entry
//   was the row's maximum).  The matrix itself is in LDS when N * C <= kProbLds, else in the workspace.
//   A suppression also writes 0 into rows that were already picked (-1 rows): the reference does, and such
//   a row can be picked again when the global maximum is 0 -- kept here, as it changes labels.
//
// prepare_pairs_kernel -- RelationSampling.prepare_test_pairs (sampling.py:31-52) for detected boxes:
//   cand = ones - eye, AND boxlist_iou(p, p) > 0 when require_overlap (boxlist_ops.py:54-89, TO_REMOVE = 1);
//   pairs in row-major order; above max_pairs the best max_pairs by pred_scores[s] * pred_scores[o] in the
//   total order (quality desc, row-major index asc) -- torch.sort(stable=True, descending=True) -- found by a
//   4 x 8-bit radix select of the max_pairs-th quality and a bitonic sort of the survivors' 64-bit keys;
//   [[0, 0]] when no pair is left.
#include "common.h"
#include "kernels.h"
#include "selection.h"

#pragma clang fp contract(off)   // the IoUs follow the reference operation for operation: a last-ulp change flips suppressions

namespace veto {

namespace {

constexpr int kMaxObj = 256;
constexpr int kProbLds = 30720;   // 120 KiB of class probabilities in LDS (80 x 151 and 100 x 201 fit; 256 x 201 does not)
constexpr int kMaxPairsCap = 4096;

// one wave: softmax of a row, its background column replaced by `bg`; returns nothing, writes prob[0..C)
__device__ __forceinline__ void wave_softmax_row(const float* __restrict__ logit, int ncls, int lane, float bg, float* prob) {
  float mx = -INFINITY;
  for (int c = lane; c < ncls; c += 64) mx = fmaxf(mx, logit[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int c = lane; c < ncls; c += 64) sum += expf(logit[c] - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int c = lane; c < ncls; c += 64) prob[c] = c == 0 ? bg : expf(logit[c] - mx) * inv;
}

// one wave: (max, first column of the max) of a row
__device__ __forceinline__ void wave_row_max(const float* prob, int ncls, int lane, float& best, int& col) {
  best = -INFINITY;
  col = 0x7fffffff;
  for (int c = lane; c < ncls; c += 64) {
    const float v = prob[c];
    if (v > best) { best = v; col = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(col, o, 64);
    if (ob > best || (ob == best && oc < col)) { best = ob; col = oc; }
  }
}

// nms_overlaps (utils_relation.py:56-92) for one (b, j) of one class, in its operation order:
// inter = clamp(min(x2) - max(x1) + 1, 0) * clamp(...y...); union = (-inter + area_j) + area_b; inter / union
__device__ __forceinline__ float nms_iou(const float* bb, const float* bj) {
  const float iw = fmaxf((fminf(bb[2], bj[2]) - fmaxf(bb[0], bj[0])) + 1.f, 0.f);
  const float ih = fmaxf((fminf(bb[3], bj[3]) - fmaxf(bb[1], bj[1])) + 1.f, 0.f);
  const float inter = iw * ih;
  const float area_b = ((bb[2] - bb[0]) + 1.f) * ((bb[3] - bb[1]) + 1.f);
  const float area_j = ((bj[2] - bj[0]) + 1.f) * ((bj[3] - bj[1]) + 1.f);
  return inter / ((-inter + area_j) + area_b);
}

__global__ __launch_bounds__(256) void obj_decode_kernel(ObjDecodeArgs a) {
  __shared__ float s_prob[kProbLds];
  __shared__ float s_rmax[kMaxObj];
  __shared__ int s_rcol[kMaxObj];
  __shared__ int s_label[kMaxObj];
  __shared__ int s_dirty[kMaxObj];
  __shared__ int s_ndirty, s_b, s_c;
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int off = a.img_off[img], n = a.img_off[img + 1] - off, C = a.n_cls;
  if (n <= 0 || n > kMaxObj) return;   // the ABI checks the host-side maximum; never index LDS past 256 rows
  const float bg = a.mode == 1 ? -1.f : 0.f;
  float* P = (size_t)n * C <= (size_t)kProbLds ? s_prob : a.prob_ws + (size_t)off * C;
  const float* boxes = a.boxes_per_cls + (size_t)off * C * 4;
  for (int r = wave; r < n; r += 4) {
    float* row = P + (size_t)r * C;
    if (a.mode == 1) {
      const int64_t lab = a.labels[off + r];
      for (int c = lane; c < C; c += 64) row[c] = c == 0 ? bg : (c == lab ? 1.f : 0.5f);
    } else {
      wave_softmax_row(a.logits + (size_t)(off + r) * C, C, lane, bg, row);
    }
    float best;
    int col;
    wave_row_max(P + (size_t)r * C, C, lane, best, col);   // each lane re-reads what it wrote itself: no barrier needed
    if (lane == 0) { s_rmax[r] = best; s_rcol[r] = col; }
  }
  for (int r = tid; r < n; r += blockDim.x) s_label[r] = 0;
  if (tid == 0) s_ndirty = 0;
  __syncthreads();
  const float thr = a.thr;
  for (int it = 0; it < n; ++it) {
    if (wave == 0) {   // global arg-max in numpy's flat order: value desc, then row asc (a row's first column is its own)
      float best = -INFINITY;
      int row = 0x7fffffff;
      for (int r = lane; r < n; r += 64) {
        const float v = s_rmax[r];
        if (v > best) { best = v; row = r; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int orow = __shfl_xor(row, o, 64);
        if (ob > best || (ob == best && orow < row)) { best = ob; row = orow; }
      }
      if (lane == 0) {
        s_b = row;
        s_c = s_rcol[row];
        if (a.mode == 1 || s_label[row] == 0) s_label[row] = s_rcol[row];
      }
    }
    __syncthreads();
    const int b = s_b, c = s_c;
    const float* bb = boxes + ((size_t)b * C + c) * 4;
    for (int j = tid; j < n; j += blockDim.x) {
      if (j == b) continue;   // row b becomes -1 below
      const float* bj = boxes + ((size_t)j * C + c) * 4;
      if (!(nms_iou(bb, bj) >= thr)) continue;
      float* pj = P + (size_t)j * C + c;
      const float old = *pj;
      if (old == 0.f) continue;
      *pj = 0.f;
      const float rm = s_rmax[j];
      const int rc = s_rcol[j];
      if (c == rc && old > 0.f) {          // the row's maximum went down: rescan
        s_dirty[atomicAdd(&s_ndirty, 1)] = j;
      } else if (0.f > rm || (0.f == rm && c < rc)) {   // a 0 in a picked (-1) row, or an earlier column at the same max
        s_rmax[j] = 0.f;
        s_rcol[j] = c;
      }
    }
    __syncthreads();
    for (int c2 = tid; c2 < C; c2 += blockDim.x) P[(size_t)b * C + c2] = -1.f;
    const int nd = s_ndirty;
    for (int k = wave; k < nd; k += 4) {
      const int r = s_dirty[k];
      float best;
      int col;
      wave_row_max(P + (size_t)r * C, C, lane, best, col);
      if (lane == 0) { s_rmax[r] = best; s_rcol[r] = col; }
    }
    if (tid == 0) { s_rmax[b] = -1.f; s_rcol[b] = 0; }
    __syncthreads();
    if (tid == 0) s_ndirty = 0;   // read above before the barrier; the next writers run after the next barrier
  }
  __syncthreads();
  // pred_scores = softmax(logits)[i, label_i] with the background column zeroed (inference.py:419-420);
  // boxes = boxes_per_cls[i, label_i] (:425-428)
  for (int r = wave; r < n; r += 4) {
    const int lab = s_label[r];
    if (lane == 0) a.obj_pred[off + r] = lab;
    if (a.out_boxes && lane < 4) a.out_boxes[(size_t)(off + r) * 4 + lane] = boxes[((size_t)r * C + lab) * 4 + lane];
    if (!a.obj_scores) continue;
    const float* logit = a.logits + (size_t)(off + r) * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, logit[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(logit[c] - mx);
    sum = wave_sum(sum);
    if (lane == 0) a.obj_scores[off + r] = lab == 0 ? 0.f : expf(logit[lab] - mx) * (1.f / sum);
  }
}

// ---- test pairs ------------------------------------------------------------------------------------

// boxlist_iou(p, p)[i, j] > 0 (boxlist_ops.py:54-89)
__device__ __forceinline__ bool boxes_overlap(const float* bi, const float* bj) { return boxlist_iou(bi, bj) > 0.f; }

__global__ __launch_bounds__(256) void prepare_pairs_kernel(PairArgs a) {
  __shared__ float s_box[kMaxObj][4];
  __shared__ float s_score[kMaxObj];
  __shared__ uint32_t s_mask[kMaxObj][8];   // bit j of row i: candidate pair (i, j)
  __shared__ unsigned long long s_key[kMaxPairsCap];
  __shared__ int s_hist[256];
  __shared__ int s_wave[4];
  __shared__ int s_nsel, s_digit, s_need;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int off = a.img_off[img], n = a.img_off[img + 1] - off;
  int64_t* out = a.pairs + 2 * (size_t)a.out_off[img];
  if (n > kMaxObj) return;   // checked on the host as well
  for (int i = tid; i < n; i += blockDim.x) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_box[i][k] = a.boxes[(size_t)(off + i) * 4 + k];
    s_score[i] = a.scores ? a.scores[off + i] : 0.f;
  }
  __syncthreads();
  // thread i owns row i: its 8 mask words and, below, its pairs in column order
  const int i = tid;
  int row_cnt = 0;
  if (i < n) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      uint32_t m = 0;
      for (int jj = 0; jj < 32; ++jj) {
        const int j = w * 32 + jj;
        if (j < n && j != i && (!a.require_overlap || boxes_overlap(s_box[i], s_box[j]))) m |= 1u << jj;
      }
      s_mask[i][w] = m;
      row_cnt += __popc(m);
    }
  }
  int total;
  const int row_base = block_exclusive_scan(row_cnt, s_wave, &total);   // its barriers also publish s_mask
  if (total == 0) {   // sampling.py:47-51 placeholder
    if (tid == 0) { out[0] = 0; out[1] = 0; a.counts[img] = 1; }
    return;
  }
  if (total <= a.max_pairs) {   // torch.nonzero order
    if (i < n) {
      int p = row_base;
      for (int w = 0; w < 8; ++w) {
        uint32_t m = s_mask[i][w];
        while (m) {
          const int j = w * 32 + __ffs(m) - 1;
          m &= m - 1;
          out[2 * (size_t)p] = i;
          out[2 * (size_t)p + 1] = j;
          ++p;
        }
      }
    }
    if (tid == 0) a.counts[img] = total;
    return;
  }
  // above the cap: the max_pairs-th largest quality T by radix select (8 bits a pass, most significant first)
  const float si = i < n ? s_score[i] : 0.f;
  uint32_t prefix = 0, pmask = 0;
  int need = a.max_pairs;   // how many of the keys matching `prefix` are still to be taken
  for (int shift = 24; shift >= 0; shift -= 8) {
    s_hist[tid] = 0;
    __syncthreads();
    if (i < n) {
      for (int w = 0; w < 8; ++w) {
        uint32_t m = s_mask[i][w];
        while (m) {
          const int j = w * 32 + __ffs(m) - 1;
          m &= m - 1;
          const uint32_t k = float_order(si * s_score[j]);   // pairs_qualities[idx0] * pairs_qualities[idx1]
          if ((k & pmask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1);
        }
      }
    }
    __syncthreads();
    // digit d: count of keys above it (digits d+1..255) < need <= that count + hist[d]
    const int h = s_hist[255 - tid];   // thread t looks at digit 255 - t: an ascending scan over descending digits
    int dummy;
    const int above = block_exclusive_scan(h, s_wave, &dummy);
    if (above < need && above + h >= need) { s_digit = 255 - tid; s_need = need - above; }
    __syncthreads();
    prefix |= (uint32_t)s_digit << shift;
    pmask |= 255u << shift;
    need = s_need;
    __syncthreads();
  }
  const uint32_t T = prefix;   // keys > T are all taken; of the keys == T the first `need` in row-major order
  int eq_cnt = 0;
  if (i < n) {
    for (int w = 0; w < 8; ++w) {
      uint32_t m = s_mask[i][w];
      while (m) {
        const int j = w * 32 + __ffs(m) - 1;
        m &= m - 1;
        eq_cnt += float_order(si * s_score[j]) == T;
      }
    }
  }
  if (tid == 0) s_nsel = 0;
  int dummy;
  int eq_rank = block_exclusive_scan(eq_cnt, s_wave, &dummy);
  if (i < n) {
    for (int w = 0; w < 8; ++w) {
      uint32_t m = s_mask[i][w];
      while (m) {
        const int j = w * 32 + __ffs(m) - 1;
        m &= m - 1;
        const uint32_t k = float_order(si * s_score[j]);
        bool take = k > T;
        if (k == T) take = eq_rank++ < need;
        if (take) {
          const int slot = atomicAdd(&s_nsel, 1);
          if (slot < kMaxPairsCap)   // exactly max_pairs are taken; never past the LDS array
            s_key[slot] = ((unsigned long long)(~k) << 32) | (unsigned)(i * n + j);
        }
      }
    }
  }
  const int cnt = a.max_pairs;
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  __syncthreads();
  for (int t = cnt + tid; t < n2; t += blockDim.x) s_key[t] = ~0ull;   // padding sorts last
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {   // ascending bitonic sort: quality desc, row-major index asc
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n2; t += blockDim.x) {
        const int l = t ^ j;
        if (l > t) {
          const unsigned long long kt = s_key[t], kl = s_key[l];
          const bool up = (t & k) == 0;
          if (up ? kt > kl : kt < kl) { s_key[t] = kl; s_key[l] = kt; }
        }
      }
      __syncthreads();
    }
  }
  for (int t = tid; t < cnt; t += blockDim.x) {
    const int flat = (int)(s_key[t] & 0xffffffffu);
    out[2 * (size_t)t] = flat / n;
    out[2 * (size_t)t + 1] = flat % n;
  }
  if (tid == 0) a.counts[img] = cnt;
}

}  // namespace

int obj_decode_max_objects() { return kMaxObj; }
int prepare_pairs_max_pairs() { return kMaxPairsCap; }

hipError_t launch_obj_decode(const ObjDecodeArgs& a, hipStream_t s) {
  VETO_LAUNCH(obj_decode_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prepare_pairs(const PairArgs& a, hipStream_t s) {
  VETO_LAUNCH(prepare_pairs_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
