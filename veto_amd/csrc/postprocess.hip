// Relation post-processing, the step right after the predicate logits:
// the vanilla, GT-box branch of PostProcessor.forward, pysgg/modeling/roi_heads/relation_head/
// inference.py:398-453.  Per image:
//   obj_prob = softmax(obj_logit); obj_prob[:, 0] = 0; obj_score, obj_pred = max over classes 1..   (:405-412)
//   rel_prob = softmax(rel_logit); rel_score, rel_class = max over classes 1..                       (:440-442)
//   triple   = rel_score * obj_score[subj] * obj_score[obj]; descending sort                         (:444-445)
//   emit rel_pair_idx, rel_prob, rel_class in that order                                              (:446-452)
// Kernels: per-object softmax/max, per-pair softmax/max/triple score (one wave per pair), one
// workgroup per image for the segmented sort (bitonic in LDS over (score desc, index asc) -- a total
// order, so the result is deterministic; torch.sort leaves the order of exact ties unspecified),
// and a row gather into sorted order.
#include "common.h"
#include "kernels.h"

namespace veto {

namespace {

// softmax statistics of a row of `n` logits, one wave: the maximum and 1 / sum of exp(logit - maximum)
__device__ __forceinline__ void wave_softmax_stats(const float* __restrict__ logit, int n, int lane, float& mx, float& inv) {
  mx = -INFINITY;
  for (int c = lane; c < n; c += 64) mx = fmaxf(mx, logit[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int c = lane; c < n; c += 64) sum += expf(logit[c] - mx);
  sum = wave_sum(sum);
  inv = 1.f / sum;
}

// arg-max across lanes of each lane's (value, class); ties -> the lower class index (torch.max)
__device__ __forceinline__ void wave_argmax(float& best, int& best_cls) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(best_cls, o, 64);
    if (ob > best || (ob == best && oc < best_cls)) { best = ob; best_cls = oc; }
  }
}

// one wave per row: softmax over `ncls` logits, then max over classes 1..ncls-1
__device__ __forceinline__ void wave_softmax_fgmax(const float* __restrict__ logit, int ncls, int lane,
                                                   float* __restrict__ prob_out, float& best, int& best_cls) {
  float mx, inv;
  wave_softmax_stats(logit, ncls, lane, mx, inv);
  best = -1.f;
  best_cls = 0x7fffffff;
  for (int c = lane; c < ncls; c += 64) {
    const float p = expf(logit[c] - mx) * inv;
    if (prob_out) prob_out[c] = p;
    if (c >= 1 && p > best) { best = p; best_cls = c; }  // first maximum inside the lane (ascending c)
  }
  wave_argmax(best, best_cls);
}

// An image's block of the batch: its first pair, pair count and first object.  With `rpp` rows per pair (1: vanilla, K: the K
// groups of the MEET merge / vote) image i owns the rows rpp * pair0 .. of rpp * pairs rows.  Null offsets: ONE image that owns
// every pair and object.
struct ImageBlock { int img, pair0, pairs, obj0; };
__device__ __forceinline__ ImageBlock image_block(const PostArgs& a, int img) {
  if (!a.img_pair_off) return ImageBlock{0, 0, a.n_pair, 0};
  const int pair0 = a.img_pair_off[img];
  return ImageBlock{img, pair0, a.img_pair_off[img + 1] - pair0, a.img_obj_off[img]};
}
// ... of the image that owns `row`: the largest i with rpp * img_pair_off[i] <= row (offsets ascending from 0; empty images share
// an offset and are skipped)
__device__ __forceinline__ ImageBlock image_block_of_row(const PostArgs& a, long row, int rpp) {
  int lo = 0, hi = a.img_pair_off ? a.n_img - 1 : 0;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long)rpp * a.img_pair_off[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return image_block(a, lo);
}

__global__ __launch_bounds__(256) void obj_score_kernel(const float* __restrict__ obj_logits, int n_obj, int ncls,
                                                        float* __restrict__ obj_scores, int64_t* __restrict__ obj_pred) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= n_obj) return;
  float best;
  int cls;
  wave_softmax_fgmax(obj_logits + (size_t)n * ncls, ncls, lane, nullptr, best, cls);
  if (lane == 0) { obj_scores[n] = best; obj_pred[n] = cls; }
}

__global__ __launch_bounds__(256) void rel_score_kernel(PostArgs a) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= a.n_pair) return;
  float best;
  int cls;
  wave_softmax_fgmax(a.rel_logits + (size_t)p * a.n_rel_cls, a.n_rel_cls, lane, a.prob_tmp + (size_t)p * a.n_rel_cls, best, cls);
  if (lane == 0) {
    const int off = image_block_of_row(a, p, 1).obj0;
    const float s0 = a.obj_scores[off + a.rel_pairs[2 * (size_t)p]];
    const float s1 = a.obj_scores[off + a.rel_pairs[2 * (size_t)p + 1]];
    a.triple[p] = best * s0 * s1;  // same association as the reference: (rel * obj0) * obj1
    a.label_tmp[p] = cls;
  }
}

// ---- the MEET merge and the expert vote ----------------------------------------------------------------------------------------
// K groups: image i owns the rows K * img_pair_off[i] .. of K * P_i rows (P_i pairs); inside that block the order before the sort
// is (group, pair), the merged list of inference.py:284-397.
// One wave per (pair, group) of the batch: grid (ceil(n_pair / 4), K).  Wave 0 derives the group's column table from the
// class -> group list: column 1 + r is the r-th class of the group.
//   merge (kVote false, inference.py:346-372): softmax over the group's g+2 logits, the last ("other group") column dropped,
//     arg-max over columns 1..g (a group-local label), the g+1 probabilities scattered into a zero num_rel_cls-wide row at
//     columns [0] + the group's own classes.
//   vote (kVote true, inference.py:93-283): three expert heads per group; a lane owns columns lane and lane + 64 of the group's
//     g+1 kept columns (g + 2 <= 105).
//     per expert e: p_e = softmax(logit_e) without its last column, (score_e, cls_e) = max over columns 1..,
//                   t_e = score_e * obj_s * obj_o                                                   (:178-190)
//     agree_ab = cls_a == cls_b for (0,1), (1,2), (0,2)                                              (:192-199)
//     consensus: pair means t_ab = (t_a + t_b)/2, p_ab = (p_a + p_b)/2 with p_12 = p_1 (the reference
//                averages expert 1 with itself, :224-226); row = sum over agreeing pairs / their count (:211-255)
//     unanimous: all three agree; row = three-way mean                                                (:257-261)
//     A voted-out row gets score -1 (it sorts behind every kept row, whose scores are >= 0) and label 0.
template <bool kVote>
__global__ __launch_bounds__(256) void group_score_kernel(PostArgs a, PostGroupTables t) {
  __shared__ int s_cols[104];
  const int k = blockIdx.y, lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    if (lane == 0) s_cols[0] = 0;
    int base = 1;
    for (int c0 = 0; c0 < a.n_rel_cls; c0 += 64) {
      const int c = c0 + lane;
      const bool mine = c < a.n_rel_cls && t.cls_group[c] == k + 1;
      const unsigned long long m = __ballot(mine);
      const int col = base + __popcll(m & ((1ull << lane) - 1ull));
      if (mine && col < 104) s_cols[col] = c;
      base += __popcll(m);
    }
  }
  __syncthreads();
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.n_pair) return;
  const ImageBlock b = image_block_of_row(a, p, 1);
  const size_t out_row = (size_t)t.n_groups * b.pair0 + (size_t)k * b.pairs + (p - b.pair0);
  const int width = t.width[k];
  float* prob = a.prob_tmp + out_row * a.n_rel_cls;
  for (int c = lane; c < a.n_rel_cls; c += 64) prob[c] = 0.f;
  const float s0 = a.obj_scores[b.obj0 + a.rel_pairs[2 * (size_t)p]];
  const float s1 = a.obj_scores[b.obj0 + a.rel_pairs[2 * (size_t)p + 1]];
  if constexpr (!kVote) {
    const float* logit = t.logits[k] + (size_t)p * width;
    float mx, inv;
    wave_softmax_stats(logit, width, lane, mx, inv);
    float best = -1.f;
    int best_cls = 0x7fffffff;
    for (int c = lane; c < width - 1; c += 64) {  // the last column is dropped
      const float pr = expf(logit[c] - mx) * inv;
      prob[s_cols[c]] = pr;
      if (c >= 1 && pr > best) { best = pr; best_cls = c; }
    }
    wave_argmax(best, best_cls);
    if (lane == 0) {
      a.triple[out_row] = best * s0 * s1;
      a.label_tmp[out_row] = best_cls;
    }
  } else {
    const int keepw = width - 1;  // the last column is dropped
    float pr[3][2], tr[3];
    int cls[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float* logit = t.logits[3 * k + e] + (size_t)p * width;
      float mx, inv;
      wave_softmax_stats(logit, width, lane, mx, inv);
      float best = -1.f;
      int best_cls = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        pr[e][j] = c < keepw ? expf(logit[c] - mx) * inv : 0.f;
        if (c >= 1 && c < keepw && pr[e][j] > best) { best = pr[e][j]; best_cls = c; }
      }
      wave_argmax(best, best_cls);
      tr[e] = best * s0 * s1;
      cls[e] = best_cls;
    }
    const bool ag01 = cls[0] == cls[1], ag12 = cls[1] == cls[2], ag02 = cls[0] == cls[2];
    float triple, out[2];
    int label;
    bool keep;
    if (t.voting == 0) {
      const int cnt = (int)ag01 + (int)ag12 + (int)ag02;
      keep = cnt > 0;
      const float fc = (float)cnt;
      triple = (((ag01 ? (tr[0] + tr[1]) * 0.5f : 0.f) + (ag12 ? (tr[1] + tr[2]) * 0.5f : 0.f)) + (ag02 ? (tr[0] + tr[2]) * 0.5f : 0.f)) / fc;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        out[j] = (((ag01 ? (pr[0][j] + pr[1][j]) * 0.5f : 0.f) + (ag12 ? (pr[1][j] + pr[1][j]) * 0.5f : 0.f)) +
                  (ag02 ? (pr[0][j] + pr[2][j]) * 0.5f : 0.f)) / fc;   // p_12 = p_1
      label = ag02 ? cls[2] : ag12 ? cls[1] : ag01 ? cls[0] : 0;  // later assignments override (:250-251)
    } else {
      keep = ag01 && ag12 && ag02;
      triple = ((tr[0] + tr[1]) + tr[2]) / 3.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) out[j] = ((pr[0][j] + pr[1][j]) + pr[2][j]) / 3.f;
      label = cls[2];
    }
    if (keep) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = lane + 64 * j;
        if (c < keepw) prob[s_cols[c]] = out[j];
      }
    }
    if (lane == 0) {
      a.triple[out_row] = keep ? triple : -1.f;
      a.label_tmp[out_row] = keep ? label : 0;
    }
  }
}

constexpr int kSortMax = 16384;  // 128 KiB of LDS: 5 MEET groups x MAX_PROPOSAL_PAIR (2048) pairs fit

// one workgroup per image: sort the rpp * P_i rows of its block by (score descending, index inside the block ascending); perm holds
// batch rows
__global__ __launch_bounds__(1024) void sort_kernel(PostArgs a, int rpp) {
  __shared__ float s_key[kSortMax];
  __shared__ int s_idx[kSortMax];
  __shared__ int s_kept;
  const ImageBlock b = image_block(a, blockIdx.x);
  const size_t r0 = (size_t)rpp * b.pair0;
  const int cnt = rpp * b.pairs;
  if (cnt > kSortMax) return;  // refused on the host; never index LDS beyond its size
  int n2 = 1;
  while (n2 < cnt) n2 <<= 1;
  for (int i = threadIdx.x; i < n2; i += blockDim.x) {
    s_key[i] = i < cnt ? a.triple[r0 + i] : -INFINITY;
    s_idx[i] = i < cnt ? i : 0x7fffffff;  // padding sorts last
  }
  if (threadIdx.x == 0) s_kept = 0;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        const int l = i ^ j;
        if (l > i) {
          const float ki = s_key[i], kl = s_key[l];
          const int ii = s_idx[i], il = s_idx[l];
          // "i before l" in the final order: higher score first, then lower index (NaN-free inputs)
          const bool i_first = ki > kl || (ki == kl && ii < il);
          const bool ascending_block = (i & k) == 0;
          if (ascending_block ? !i_first : i_first) {
            s_key[i] = kl; s_key[l] = ki;
            s_idx[i] = il; s_idx[l] = ii;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) a.perm[r0 + i] = (int)r0 + s_idx[i];
  if (a.kept_count) {  // voted-out rows carry score -1 and sort last: the kept rows are a prefix of the block
    int mine = 0;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) mine += s_key[i] >= 0.f;
    if (mine) atomicAdd(&s_kept, mine);
    __syncthreads();
    if (threadIdx.x == 0) a.kept_count[b.img] = s_kept;
  }
}

// one wave per output row: the source row from perm; its pair is the row itself (rpp 1) or, inside the image's block, the local
// source row % P_img (K copies of the image's pair list)
__global__ __launch_bounds__(256) void gather_kernel(PostArgs a, int rpp) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= (long)rpp * a.n_pair) return;
  const size_t src = a.perm[r];
  for (int c = lane; c < a.n_rel_cls; c += 64) a.out_prob[(size_t)r * a.n_rel_cls + c] = a.prob_tmp[src * a.n_rel_cls + c];
  if (lane == 0) {
    size_t psrc = src;
    if (rpp > 1) {  // (uniform: the vanilla gather makes no image search)
      const ImageBlock b = image_block_of_row(a, r, rpp);
      psrc = (size_t)b.pair0 + (src - (size_t)rpp * b.pair0) % b.pairs;
    }
    a.out_pairs[2 * (size_t)r] = a.rel_pairs[2 * psrc];
    a.out_pairs[2 * (size_t)r + 1] = a.rel_pairs[2 * psrc + 1];
    a.out_labels[r] = a.label_tmp[src];
    if (a.out_triple) a.out_triple[r] = a.triple[src];
  }
}

}  // namespace

int postprocess_max_pairs_per_image() { return kSortMax; }

// obj_logits == nullptr (sgdet): obj_scores / obj_pred were filled by the object decoding (sgdet.hip) and are inputs here
hipError_t launch_postprocess(const PostArgs& a, const PostGroupTables* t, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (a.obj_logits) {
    VETO_LAUNCH(obj_score_kernel, dim3((a.n_obj + 3) / 4), dim3(256), 0, s, a.obj_logits, a.n_obj, a.n_obj_cls, a.obj_scores, a.obj_pred);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int rpp = t ? t->n_groups : 1;
  const dim3 score_grid((a.n_pair + 3) / 4, rpp);
  if (!t) VETO_LAUNCH(rel_score_kernel, score_grid, dim3(256), 0, s, a);
  else if (t->experts == 3) VETO_LAUNCH(group_score_kernel<true>, score_grid, dim3(256), 0, s, a, *t);
  else VETO_LAUNCH(group_score_kernel<false>, score_grid, dim3(256), 0, s, a, *t);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  VETO_LAUNCH(sort_kernel, dim3(a.n_img), dim3(1024), 0, s, a, rpp);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const long rows = (long)rpp * a.n_pair;
  VETO_LAUNCH(gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a, rpp);
  return hipGetLastError();
}

}  // namespace veto
