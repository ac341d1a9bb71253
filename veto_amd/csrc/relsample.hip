// SGDet training: RelationSampling.detect_relsample (pysgg/modeling/roi_heads/relation_head/sampling.py:109-176) with
// motif_rel_fg_bg_sampling (:179-309), one workgroup (256 threads) per image.  The reference loops over the GT relations
// of an image on the host with several device synchronisations per relation; here the whole batch is one launch.
//
//   matching     ious = boxlist_iou(target, proposal); is_match = same label & iou > fg_thres; locating_match[p] = any
//                target with iou > fg_thres.  Bit masks in LDS: s_match[t] (which proposals match target t).
//   candidates   rel_possibility = ones - eye, or 0 < boxlist_iou(p, p) < 1 with require_overlap; rows and columns of
//                proposals labelled 0 cleared.  Bit masks s_poss[i].
//   foreground   GT relations in nonzero(relation) order, 256 matrix entries per step, one thread per relation: its
//                candidates are (matches of h) x (matches of t) head-major without self-pairs; all of them leave
//                s_poss; above per_rel it draws per_rel with probability proportional to iou[h, p_h] * iou[t, p_t]
//                without replacement (npr.choice) as Efraimidis-Spirakis keys log(u) / w, largest first -- the same
//                distribution, draw order included.  binary_rel gets (head matches) x (tail matches) both ways.
//                A block scan of the per-relation counts places every relation's triplets (relation order).
//                Above max_fg triplets: a uniformly random max_fg of them in random order (randperm[:max_fg]), as the
//                max_fg smallest 32-bit hashes, sorted.
//   background   the surviving candidates; num_neg = min(batch - n_fg, n_bg); the window is the first 2 * num_neg by
//                (score[s] * score[o] desc, row-major index asc), a radix select as in prepare_pairs_kernel; of the
//                window a uniformly random num_neg in random order (randperm[:num_neg]), again by hash keys.
//   degenerate   no foreground and no background: two (0, 0, 0) rows (:298-304).
//   labels_all   with relation_non_masked: the label of nonzero(relation_non_masked)[i] for each triplet relation i
//                produced before the cap (:160-167), then zeros for the background rows; an index past the end of that
//                list sets status bit 1 instead of being clamped.
// Randomness: a counter-based hash of (seed, image, purpose, element), so an image's draws depend only on the seed,
// its index and its own inputs.
#include "common.h"
#include "kernels.h"
#include "selection.h"

namespace veto {

namespace {

constexpr int kMaxObj = 256;     // DETECTIONS_PER_IMG and GT boxes per image: one thread per row, 8 mask words per row
constexpr int kMaxBatch = 2048;  // BATCH_SIZE_PER_IMAGE: the sort buffer holds one selection
constexpr int kMaxPerRel = 16;   // NUM_SAMPLE_PER_GT_REL: the per-thread draw list lives in registers

enum { kDrawFg = 0, kCapFg = 1, kPickBg = 2 };

__global__ __launch_bounds__(256) void detect_relsample_kernel(RelSampleArgs a) {
  __shared__ float s_pbox[kMaxObj][4];
  __shared__ float s_tbox[kMaxObj][4];
  __shared__ int64_t s_plab[kMaxObj];
  __shared__ float s_score[kMaxObj];
  __shared__ uint32_t s_match[kMaxObj][8];   // bit p of row t: is_match[t, p]
  __shared__ uint32_t s_poss[kMaxObj][8];    // bit j of row i: rel_possibility[i, j]
  __shared__ uint32_t s_bin[kMaxObj][8];     // bit j of row i: binary_rel[i, j]
  __shared__ uint32_t s_loc[8];
  __shared__ unsigned long long s_key[kMaxBatch];
  __shared__ SelLds s_sel;
  __shared__ int s_nsel, s_status;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int poff = a.prp_off[img], np = a.prp_off[img + 1] - poff;
  const int toff = a.tgt_off[img], nt = a.tgt_off[img + 1] - toff;
  const int roff = a.rel_off[img];
  if (np > kMaxObj || nt > kMaxObj) return;   // the ABI checks the host-side maxima; never index LDS past 256 rows
  const int64_t* rel = a.relation + roff;
  int64_t* nm_lab = a.ws_nm + roff;
  uint32_t* fg = a.ws_fg + (size_t)roff * a.per_rel;
  int64_t* out_pairs = a.pairs + 2 * (size_t)img * a.out_rows;
  int64_t* out_labels = a.labels + (size_t)img * a.out_rows;
  int64_t* out_all = a.labels_all ? a.labels_all + (size_t)roff * a.per_rel + (size_t)img * a.out_rows : nullptr;
  const float thr = a.fg_thres;

  for (int i = tid; i < kMaxObj; i += blockDim.x) {
    if (i < np) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_pbox[i][k] = a.prp_boxes[(size_t)(poff + i) * 4 + k];
      s_plab[i] = a.prp_labels[poff + i];
      s_score[i] = a.prp_scores[poff + i];
    }
    if (i < nt) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s_tbox[i][k] = a.tgt_boxes[(size_t)(toff + i) * 4 + k];
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) s_bin[i][w] = 0;
  }
  if (tid < 8) s_loc[tid] = 0;
  if (tid == 0) s_status = 0;
  __syncthreads();

  // matching: thread t owns target row t
  if (tid < nt) {
    const int64_t tl = a.tgt_labels[toff + tid];
    for (int w = 0; w < 8; ++w) {
      uint32_t m = 0, loc = 0;
      for (int jj = 0; jj < 32; ++jj) {
        const int p = w * 32 + jj;
        if (p >= np) break;
        if (boxlist_iou(s_tbox[tid], s_pbox[p]) > thr) {
          loc |= 1u << jj;
          if (s_plab[p] == tl) m |= 1u << jj;
        }
      }
      s_match[tid][w] = m;
      if (loc) atomicOr(&s_loc[w], loc);
    }
  }
  // candidates: thread i owns proposal row i
  if (tid < np) {
    const int i = tid;
    for (int w = 0; w < 8; ++w) {
      uint32_t m = 0;
      if (s_plab[i] != 0) {
        for (int jj = 0; jj < 32; ++jj) {
          const int j = w * 32 + jj;
          if (j >= np) break;
          if (j == i || s_plab[j] == 0) continue;
          if (a.require_overlap) {
            const float iou = boxlist_iou(s_pbox[i], s_pbox[j]);
            if (!(iou > 0.f && iou < 1.f)) continue;
          }
          m |= 1u << jj;
        }
      }
      s_poss[i][w] = m;
    }
  }
  __syncthreads();
  for (int p = tid; p < np; p += blockDim.x) a.locating[poff + p] = (s_loc[p >> 5] >> (p & 31)) & 1u ? 1.f : 0.f;

  const int TT = nt * nt;
  // labels of nonzero(relation_non_masked), by rank
  int m_total = 0;
  if (a.relation_nm) {
    for (int base = 0; base < TT; base += blockDim.x) {
      const int e = base + tid;
      const int64_t v = e < TT ? a.relation_nm[roff + e] : 0;
      int tot;
      const int r = block_exclusive_scan(v != 0, s_sel.wave, &tot);
      if (v != 0) nm_lab[m_total + r] = v;
      m_total += tot;
    }
  }
  __syncthreads();   // nm_lab is read below by other threads (global memory, same workgroup)

  // foreground: one thread per relation, 256 matrix entries per step
  const int per_rel = a.per_rel;
  int rel_base = 0, fg_base = 0;
  for (int base = 0; base < TT; base += blockDim.x) {
    const int e = base + tid;
    const int64_t lab = e < TT ? rel[e] : 0;
    const bool is_rel = lab != 0;
    const int h = is_rel ? e / nt : 0, t = is_rel ? e % nt : 0;
    int nh = 0, ntl = 0, nc = 0, f = 0;
    if (is_rel) {
      int nself = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        nh += __popc(s_match[h][w]);
        ntl += __popc(s_match[t][w]);
        nself += __popc(s_match[h][w] & s_match[t][w]);
      }
      nc = nh * ntl - nself;
      f = min(nc, per_rel);
    }
    int tot_rel, tot_f;
    const int rank = rel_base + block_exclusive_scan(is_rel ? 1 : 0, s_sel.wave, &tot_rel);
    const int off = fg_base + block_exclusive_scan(f, s_sel.wave, &tot_f);
    if (nh > 0 && ntl > 0) {   // binary_rel: (head matches) x (tail matches), both ways, self entries included
      for (int w = 0; w < 8; ++w) {
        uint32_t m = s_match[h][w];
        while (m) {
          const int ph = w * 32 + __ffs(m) - 1;
          m &= m - 1;
          for (int w2 = 0; w2 < 8; ++w2)
            if (s_match[t][w2]) atomicOr(&s_bin[ph][w2], s_match[t][w2]);
        }
        m = s_match[t][w];
        while (m) {
          const int pt = w * 32 + __ffs(m) - 1;
          m &= m - 1;
          for (int w2 = 0; w2 < 8; ++w2)
            if (s_match[h][w2]) atomicOr(&s_bin[pt][w2], s_match[h][w2]);
        }
      }
    }
    if (nc > 0) {   // every candidate leaves rel_possibility (self-pairs are never candidates there)
      for (int w = 0; w < 8; ++w) {
        uint32_t m = s_match[h][w];
        while (m) {
          const int ph = w * 32 + __ffs(m) - 1;
          m &= m - 1;
          for (int w2 = 0; w2 < 8; ++w2)
            if (s_match[t][w2]) atomicAnd(&s_poss[ph][w2], ~s_match[t][w2]);
        }
      }
    }
    if (f > 0) {
      float bk[kMaxPerRel];
      uint32_t bp[kMaxPerRel];
#pragma unroll
      for (int s = 0; s < kMaxPerRel; ++s) { bk[s] = -INFINITY; bp[s] = 0; }
      float floor_k = -INFINITY;
      int idx = 0;
      for (int w = 0; w < 8; ++w) {
        uint32_t mh = s_match[h][w];
        while (mh) {
          const int ph = w * 32 + __ffs(mh) - 1;
          mh &= mh - 1;
          const float iou_h = boxlist_iou(s_tbox[h], s_pbox[ph]);
          for (int w2 = 0; w2 < 8; ++w2) {
            uint32_t mt = s_match[t][w2];
            while (mt) {
              const int pt = w2 * 32 + __ffs(mt) - 1;
              mt &= mt - 1;
              if (pt == ph) continue;
              const uint32_t packed = (uint32_t)ph | ((uint32_t)pt << 8) | ((uint32_t)e << 16);
              if (nc <= per_rel) {   // all of them, in candidate order
                fg[off + idx++] = packed;
                continue;
              }
              const float wgt = iou_h * boxlist_iou(s_tbox[t], s_pbox[pt]);
              const uint64_t r = rng64(a.seed, img, kDrawFg, packed);
              const float u = ((float)(uint32_t)(r >> 40) + 0.5f) * 5.9604645e-08f;   // (0, 1), 24 bits
              float ck = logf(u) / wgt;
              if (!(ck > floor_k)) continue;
              uint32_t cp = packed;
#pragma unroll
              for (int s = 0; s < kMaxPerRel; ++s) {
                if (s < per_rel && ck > bk[s]) {
                  const float tk = bk[s];
                  const uint32_t tp = bp[s];
                  bk[s] = ck; bp[s] = cp; ck = tk; cp = tp;
                }
              }
#pragma unroll
              for (int s = 0; s < kMaxPerRel; ++s)
                if (s == per_rel - 1) floor_k = bk[s];
            }
          }
        }
      }
      if (nc > per_rel) {
#pragma unroll
        for (int s = 0; s < kMaxPerRel; ++s)
          if (s < per_rel) fg[off + s] = bp[s];
      }
      if (out_all) {
        int64_t v = 0;
        if (rank < m_total) v = nm_lab[rank];
        else atomicOr(&s_status, 1);
        for (int s = 0; s < f; ++s) out_all[off + s] = v;
      }
    }
    rel_base += tot_rel;
    fg_base += tot_f;
  }
  __syncthreads();   // s_poss, s_bin final; fg[] written by other threads
  const int F = fg_base;
  const int n_fg = min(F, a.max_fg);

  // foreground cap
  if (F <= a.max_fg) {
    for (int s = tid; s < F; s += blockDim.x) {
      const uint32_t pk = fg[s];
      const int e = (int)(pk >> 16);
      out_pairs[2 * (size_t)s] = pk & 255u;
      out_pairs[2 * (size_t)s + 1] = (pk >> 8) & 255u;
      out_labels[s] = rel[e];
    }
  } else if (n_fg > 0) {
    const int chunk = (F + blockDim.x - 1) / blockDim.x;
    const int e0 = min(F, tid * chunk), e1 = min(F, e0 + chunk);
    auto each = [&](auto f) {
      for (int e = e0; e < e1; ++e) f(~(uint32_t)(rng64(a.seed, img, kCapFg, (uint32_t)e) >> 32));
    };
    uint32_t T;
    int need;
    radix_select(each, n_fg, s_sel, T, need);
    int eq = equal_rank(each, T, s_sel);
    if (tid == 0) s_nsel = 0;
    __syncthreads();
    for (int e = e0; e < e1; ++e) {
      const uint32_t k = ~(uint32_t)(rng64(a.seed, img, kCapFg, (uint32_t)e) >> 32);
      bool take = k > T;
      if (k == T) take = eq++ < need;
      if (take) {
        const int slot = atomicAdd(&s_nsel, 1);
        if (slot < kMaxBatch) s_key[slot] = ((unsigned long long)(~k) << 32) | (uint32_t)e;
      }
    }
    __syncthreads();
    bitonic_sort(s_key, n_fg);
    for (int s = tid; s < n_fg; s += blockDim.x) {
      const uint32_t pk = fg[(uint32_t)(s_key[s] & 0xffffffffu)];
      out_pairs[2 * (size_t)s] = pk & 255u;
      out_pairs[2 * (size_t)s + 1] = (pk >> 8) & 255u;
      out_labels[s] = rel[pk >> 16];
    }
    __syncthreads();   // s_key is reused below
  }

  // background: thread i owns candidate row i
  const int i = tid;
  int row_cnt = 0;
  if (i < np) {
#pragma unroll
    for (int w = 0; w < 8; ++w) row_cnt += __popc(s_poss[i][w]);
  }
  int n_bg;
  (void)block_exclusive_scan(row_cnt, s_sel.wave, &n_bg);
  const int num_neg = min(a.batch - n_fg, n_bg);
  const int win = min(2 * num_neg, n_bg);
  const float si = i < np ? s_score[i] : 0.f;
  auto each_q = [&](auto f) {   // window keys: pairs_qualities
    if (i >= np) return;
    for (int w = 0; w < 8; ++w) {
      uint32_t m = s_poss[i][w];
      while (m) {
        const int j = w * 32 + __ffs(m) - 1;
        m &= m - 1;
        f(float_order(si * s_score[j]));
      }
    }
  };
  uint32_t Tq = 0;
  int need_q = 0, rq0 = 0;
  if (num_neg > 0 && win < n_bg) {
    radix_select(each_q, win, s_sel, Tq, need_q);
    rq0 = equal_rank(each_q, Tq, s_sel);
  }
  const bool whole = win == n_bg;
  // visits the window members of row i in row order: f(hash key, flat index)
  auto each_win = [&](auto f) {
    if (i >= np) return;
    int rq = rq0;
    for (int w = 0; w < 8; ++w) {
      uint32_t m = s_poss[i][w];
      while (m) {
        const int j = w * 32 + __ffs(m) - 1;
        m &= m - 1;
        bool in = whole;
        if (!in) {
          const uint32_t kq = float_order(si * s_score[j]);
          in = kq > Tq;
          if (kq == Tq) in = rq++ < need_q;
        }
        if (!in) continue;
        const uint32_t flat = (uint32_t)(i * np + j);
        f(~(uint32_t)(rng64(a.seed, img, kPickBg, flat) >> 32), flat);
      }
    }
  };
  if (num_neg > 0) {
    uint32_t T2 = 0;
    int need2 = 0, r2 = 0;
    const bool all = num_neg == win;
    if (!all) {
      auto each_h = [&](auto f) { each_win([&](uint32_t k, uint32_t) { f(k); }); };
      radix_select(each_h, num_neg, s_sel, T2, need2);
      r2 = equal_rank(each_h, T2, s_sel);
    }
    if (tid == 0) s_nsel = 0;
    __syncthreads();
    each_win([&](uint32_t k, uint32_t flat) {
      bool take = all || k > T2;
      if (!all && k == T2) take = r2++ < need2;
      if (take) {
        const int slot = atomicAdd(&s_nsel, 1);
        if (slot < kMaxBatch) s_key[slot] = ((unsigned long long)(~k) << 32) | flat;
      }
    });
    __syncthreads();
    bitonic_sort(s_key, num_neg);
    for (int s = tid; s < num_neg; s += blockDim.x) {
      const int flat = (int)(s_key[s] & 0xffffffffu);
      out_pairs[2 * (size_t)(n_fg + s)] = flat / np;
      out_pairs[2 * (size_t)(n_fg + s) + 1] = flat % np;
      out_labels[n_fg + s] = 0;
    }
  }
  const int rows = (n_fg == 0 && num_neg == 0) ? 2 : n_fg + num_neg;
  for (int s = n_fg + num_neg + tid; s < rows; s += blockDim.x) {   // :298-304
    out_pairs[2 * (size_t)s] = 0;
    out_pairs[2 * (size_t)s + 1] = 0;
    out_labels[s] = 0;
  }
  if (out_all)
    for (int s = tid; s < rows - n_fg; s += blockDim.x) out_all[F + s] = 0;
  for (int idx = tid; idx < np * np; idx += blockDim.x) {
    const int r = idx / np, c = idx % np;
    a.binary[(size_t)a.bin_off[img] + idx] = (s_bin[r][c >> 5] >> (c & 31)) & 1u;
  }
  __syncthreads();   // s_status
  if (tid == 0) {
    int32_t* cnt = a.counts + 4 * (size_t)img;
    cnt[0] = rows;
    cnt[1] = F;
    cnt[2] = n_fg;
    cnt[3] = s_status;
  }
}

}  // namespace

int relsample_max_objects() { return kMaxObj; }
int relsample_max_batch() { return kMaxBatch; }
int relsample_max_per_rel() { return kMaxPerRel; }

hipError_t launch_detect_relsample(const RelSampleArgs& a, hipStream_t s) {
  VETO_LAUNCH(detect_relsample_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
