// predcls / sgcls training: RelationSampling.gtbox_relsample (pysgg/modeling/roi_heads/relation_head/sampling.py:54-107), one
// workgroup (256 threads) per image.  The reference loops over the images on the host, about fifteen small launches and four
// nonzero / index synchronisations each; here the whole batch is one launch.
//
//   matrix       relation [n, n] is read once, coalesced: bit (h, t) of s_fg = relation[h, t] > 0 (:62), s_bin gets (h, t) and
//                (t, h) (binary_rel, :77-80, before any cap).  Labels are re-read from the matrix for the rows that are kept.
//   candidates   never materialised.  Thread t owns the cells [t * chunk, (t + 1) * chunk) of the row-major matrix, so the
//                threads' candidates are consecutive ranges in torch.nonzero order: foreground = the bit is set, background
//                = off the diagonal and the bit is clear (:82-85, only that direction is excluded).
//   foreground   m_fg <= num_pos: all of them in row-major order (a block scan of the per-thread counts places them).
//                Above: a uniformly random num_pos of them in random order (randperm(m)[:k], :88-91).
//   background   min(m_bg, batch - n_fg) of them, a uniformly random subset in random order (:94-96), also when all are taken.
// A random subset of size K: every candidate gets the upper 32 bits of rng64(seed, image, purpose, flat cell index); the K
// smallest (hash, index) are found by a radix select over keys computed on the fly, then sorted, ascending.  An image's draws
// depend only on the seed, its index in the batch and its own matrix.
#include "common.h"
#include "kernels.h"
#include "selection.h"

namespace veto {

namespace {

constexpr int kMaxObj = 256;     // GT boxes per image: 8 mask words per row
constexpr int kMaxBatch = 2048;  // BATCH_SIZE_PER_IMAGE: the sort buffer holds one selection

enum { kPickFg = 0, kPickBg = 1 };

// The K of M candidates (0 < K <= M, K <= kMaxBatch) with the smallest (hash, index), sorted, into s_key[0..K) as
// (hash << 32) | index.  each(f) calls f(~hash, index) for this thread's candidates in index order.
template <class Each>
__device__ void pick_smallest(Each each, int K, int M, unsigned long long* s_key, SelLds& s_sel, int* s_nsel) {
  uint32_t T = 0;
  int need = 0, eq = 0;
  const bool all = K == M;
  if (!all) {
    auto keys = [&](auto f) { each([&](uint32_t k, uint32_t) { f(k); }); };
    radix_select(keys, K, s_sel, T, need);
    eq = equal_rank(keys, T, s_sel);
  }
  if (threadIdx.x == 0) *s_nsel = 0;
  __syncthreads();
  each([&](uint32_t k, uint32_t e) {
    bool take = all || k > T;
    if (!all && k == T) take = eq++ < need;
    if (take) {
      const int slot = atomicAdd(s_nsel, 1);
      if (slot < kMaxBatch) s_key[slot] = ((unsigned long long)(~k) << 32) | e;
    }
  });
  __syncthreads();
  bitonic_sort(s_key, K);
}

__global__ __launch_bounds__(256) void gtbox_relsample_kernel(GtboxRelSampleArgs a) {
  __shared__ uint32_t s_fg[kMaxObj][8];    // bit t of row h: relation[h, t] > 0
  __shared__ uint32_t s_bin[kMaxObj][8];   // bit j of row i: binary_rel[i, j]
  __shared__ unsigned long long s_key[kMaxBatch];
  __shared__ SelLds s_sel;
  __shared__ int s_nsel;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int n = a.obj_off[img + 1] - a.obj_off[img];
  const int roff = a.rel_off[img];
  int32_t* cnt = a.counts + 2 * (size_t)img;
  if (n <= 0 || n > kMaxObj) {   // the ABI checks the host-side maximum; never index LDS past 256 rows
    if (tid == 0) cnt[0] = cnt[1] = 0;
    return;
  }
  const int64_t* rel = a.relation + roff;
  int64_t* out_pairs = a.pairs + 2 * (size_t)img * a.batch;
  int64_t* out_labels = a.labels + (size_t)img * a.batch;
  const int NN = n * n;

  for (int i = tid; i < n; i += blockDim.x) {
#pragma unroll
    for (int w = 0; w < 8; ++w) { s_fg[i][w] = 0; s_bin[i][w] = 0; }
  }
  __syncthreads();
  for (int e = tid; e < NN; e += blockDim.x) {
    if (rel[e] > 0) {
      const int h = e / n, t = e - h * n;
      atomicOr(&s_fg[h][t >> 5], 1u << (t & 31));
      atomicOr(&s_bin[h][t >> 5], 1u << (t & 31));
      atomicOr(&s_bin[t][h >> 5], 1u << (h & 31));
    }
  }
  __syncthreads();
  for (int e = tid; e < NN; e += blockDim.x) {
    const int r = e / n, c = e - r * n;
    a.binary[(size_t)roff + e] = (s_bin[r][c >> 5] >> (c & 31)) & 1u;
  }

  // this thread's cells, in row-major order: f(flat index, row, column, is foreground)
  const int chunk = (NN + blockDim.x - 1) / blockDim.x;
  const int e0 = min(NN, tid * chunk), e1 = min(NN, e0 + chunk);
  const int r0 = e0 / n, c0 = e0 - r0 * n;
  auto cells = [&](auto f) {
    int r = r0, c = c0;
    for (int e = e0; e < e1; ++e) {
      f(e, r, c, ((s_fg[r][c >> 5] >> (c & 31)) & 1u) != 0);
      if (++c == n) { c = 0; ++r; }
    }
  };
  int my_fg = 0, my_bg = 0;
  cells([&](int, int r, int c, bool fg) {
    my_fg += fg;
    my_bg += !fg && r != c;
  });
  int m_fg, m_bg;
  const int fg_rank = block_exclusive_scan(my_fg, s_sel.wave, &m_fg);
  (void)block_exclusive_scan(my_bg, s_sel.wave, &m_bg);

  // foreground
  const int n_fg = min(m_fg, a.num_pos);
  if (m_fg <= a.num_pos) {
    int s = fg_rank;
    cells([&](int e, int r, int c, bool fg) {
      if (!fg || s >= a.batch) return;
      out_pairs[2 * (size_t)s] = r;
      out_pairs[2 * (size_t)s + 1] = c;
      out_labels[s] = rel[e];
      ++s;
    });
  } else if (n_fg > 0) {
    auto each = [&](auto f) {
      cells([&](int e, int, int, bool fg) {
        if (fg) f(~(uint32_t)(rng64(a.seed, img, kPickFg, (uint32_t)e) >> 32), (uint32_t)e);
      });
    };
    pick_smallest(each, n_fg, m_fg, s_key, s_sel, &s_nsel);
    for (int s = tid; s < n_fg; s += blockDim.x) {
      const int e = (int)(s_key[s] & 0xffffffffu);
      out_pairs[2 * (size_t)s] = e / n;
      out_pairs[2 * (size_t)s + 1] = e % n;
      out_labels[s] = rel[e];
    }
    __syncthreads();   // s_key is reused below
  }

  // background
  const int n_bg = min(m_bg, a.batch - n_fg);
  if (n_bg > 0) {
    auto each = [&](auto f) {
      cells([&](int e, int r, int c, bool fg) {
        if (!fg && r != c) f(~(uint32_t)(rng64(a.seed, img, kPickBg, (uint32_t)e) >> 32), (uint32_t)e);
      });
    };
    pick_smallest(each, n_bg, m_bg, s_key, s_sel, &s_nsel);
    for (int s = tid; s < n_bg; s += blockDim.x) {
      const int e = (int)(s_key[s] & 0xffffffffu);
      out_pairs[2 * (size_t)(n_fg + s)] = e / n;
      out_pairs[2 * (size_t)(n_fg + s) + 1] = e % n;
      out_labels[n_fg + s] = 0;
    }
  }
  if (tid == 0) {
    cnt[0] = n_fg;
    cnt[1] = n_bg;
  }
}

}  // namespace

int gtbox_relsample_max_objects() { return kMaxObj; }
int gtbox_relsample_max_batch() { return kMaxBatch; }

hipError_t launch_gtbox_relsample(const GtboxRelSampleArgs& a, hipStream_t s) {
  VETO_LAUNCH(gtbox_relsample_kernel, dim3(a.n_img), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace veto
